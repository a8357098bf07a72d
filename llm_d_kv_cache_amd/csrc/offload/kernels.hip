// CDNA4 (gfx950) kernels for the KV-block data plane.
//
// Replaces the reference's byte-wise copy_blocks_kernel + per-layer launch
// loop (csrc/storage/tensor_copier_kernels.cu:54-151) with an MI355X-first
// design:
//   - one launch covers ALL (block, layer) tiles of a file transfer;
//   - 16 B/lane vectorized copies (dwordx4), wave64-shaped;
//   - LARGE tiles: 2D grid, tile on blockIdx.x (the unbounded dimension —
//     consecutive tiles land on consecutive XCDs via the b%8 placement),
//     slice on blockIdx.y, grid-stride inside the tile;
//     (a flat-grid variant with magic-division tile lookup was measured
//     SLOWER for small tiles than this 2D shape — per-vector mapping
//     overhead at 2.3 TB/s vs 5.4-6.6 TB/s for the sliced 2D fp8 kernels
//     at the same 8 KiB x 80-layer geometry; rocprof table in
//     profiles/r02 — so every tile size uses the 2D grid);
//   - gather destination is contiguous staging, so the PCIe hop can run on
//     the SDMA engines (hipMemcpyAsync) with zero CU occupancy, or the
//     kernel can write device-mapped pinned host memory directly
//     (zero-copy mode) — the engine chooses per config.
//
// Block ids travel by value (kernarg) up to kMaxBlocksPerFile; bigger
// transfers pass a device pointer (ids_dev) instead, so there is no hard
// ceiling on blocks-per-file from the kernel side.
//
// A batched prefix-hash kernel (FNV-64a over canonical CBOR, one lane per
// sequence) accelerates bulk block-key computation for event floods.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kvo {

constexpr int kMaxBlocksPerFile = 128;   // by-value kernarg limit
constexpr int kMaxBlocksPerFileDev = 4096;  // via ids_dev device pointer

struct BlockList {
  int32_t ids[kMaxBlocksPerFile];
};

__device__ __forceinline__ int32_t block_id(const BlockList& bl,
                                            const int32_t* __restrict__ ids_dev,
                                            int bi) {
  return ids_dev != nullptr ? ids_dev[bi] : bl.ids[bi];
}

// ---- gather / scatter (large tiles: 2D grid) --------------------------------
// Tile (bi, l): block_bytes contiguous bytes.
//   device side: layer_ptrs[l] + ids[bi] * layer_strides[l]
//   staging side: dst + (bi * num_layers + l) * (block_bytes + footer_bytes)
// footer_bytes is 0 for today's dense layout and 16 when records carry a
// checksum footer (see kvc_seal_records below); every gather/scatter kernel
// takes it as its last argument and only the record stride depends on it.
// Grid: x = tile index, y = slices per tile (grid-stride inside the tile).
// 16-byte vectors; block_bytes % 16 == 0 (host-checked).

__global__ __launch_bounds__(256) void kvc_gather_blocks(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, uint8_t* __restrict__ dst,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  uint4* __restrict__ out = reinterpret_cast<uint4*>(
      dst + static_cast<uint64_t>(tile) * (block_bytes + footer_bytes));
  const uint64_t nvec = block_bytes / 16;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride)
    out[v] = src[v];
}

__global__ __launch_bounds__(256) void kvc_scatter_blocks(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, const uint8_t* __restrict__ src,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  uint4* __restrict__ out = reinterpret_cast<uint4*>(
      static_cast<uint8_t*>(const_cast<void*>(layer_ptrs[l])) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint4* __restrict__ in = reinterpret_cast<const uint4*>(
      src + static_cast<uint64_t>(tile) * (block_bytes + footer_bytes));
  const uint64_t nvec = block_bytes / 16;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride)
    out[v] = in[v];
}

// ---- batched prefix hashing -------------------------------------------------
// One lane per sequence: walks the chain hash_{c+1} = FNV64a(CBOR([h_c,
// chunk, null])). Sequences share a flat token buffer with offsets.
// Text extras (multimodal) stay on the CPU path.

__device__ __forceinline__ uint64_t fnv_byte(uint64_t h, uint8_t b) {
  return (h ^ b) * 0x100000001b3ull;
}

__device__ __forceinline__ uint64_t fnv_uint_cbor(uint64_t h, uint64_t v,
                                                  uint8_t major) {
  const uint8_t m = major << 5;
  if (v < 24) return fnv_byte(h, m | static_cast<uint8_t>(v));
  if (v <= 0xff) return fnv_byte(fnv_byte(h, m | 24), static_cast<uint8_t>(v));
  if (v <= 0xffff) {
    h = fnv_byte(h, m | 25);
    h = fnv_byte(h, static_cast<uint8_t>(v >> 8));
    return fnv_byte(h, static_cast<uint8_t>(v));
  }
  if (v <= 0xffffffffull) {
    h = fnv_byte(h, m | 26);
    for (int s = 24; s >= 0; s -= 8) h = fnv_byte(h, static_cast<uint8_t>(v >> s));
    return h;
  }
  h = fnv_byte(h, m | 27);
  for (int s = 56; s >= 0; s -= 8) h = fnv_byte(h, static_cast<uint8_t>(v >> s));
  return h;
}

__global__ void kvc_prefix_hash(
    const uint32_t* __restrict__ tokens,   // flat token buffer
    const uint64_t* __restrict__ seq_off,  // [n_seq + 1] offsets into tokens
    const uint64_t* __restrict__ seeds,    // [n_seq] chain seeds (parent or model seed)
    uint64_t* __restrict__ keys,           // flat key buffer
    const uint64_t* __restrict__ key_off,  // [n_seq + 1] offsets into keys
    int block_size, int n_seq) {
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seq) return;
  const uint32_t* t = tokens + seq_off[s];
  const uint64_t n_tokens = seq_off[s + 1] - seq_off[s];
  const uint64_t n_chunks = n_tokens / block_size;
  uint64_t* out = keys + key_off[s];
  uint64_t prefix = seeds[s];
  for (uint64_t c = 0; c < n_chunks; ++c) {
    uint64_t h = 0xcbf29ce484222325ull;
    h = fnv_byte(h, 0x83);                       // array(3)
    h = fnv_uint_cbor(h, prefix, 0);             // parent
    h = fnv_uint_cbor(h, block_size, 4);         // array(block_size)
    for (int i = 0; i < block_size; ++i)
      h = fnv_uint_cbor(h, t[c * block_size + i], 0);
    h = fnv_byte(h, 0xf6);                       // null extra
    prefix = h;
    out[c] = h;
  }
}

// ---- launchers --------------------------------------------------------------

inline dim3 copy_grid(uint32_t tiles, uint64_t block_bytes) {
  // Fill the chip: >= 2048 workgroups when the transfer is large enough.
  uint64_t vec_per_tile = block_bytes / 16;
  uint32_t max_wg_per_tile =
      static_cast<uint32_t>((vec_per_tile + 255) / 256);  // cap: 1 vec/lane
  uint32_t want = tiles >= 2048 ? 1 : (2048 + tiles - 1) / tiles;
  uint32_t wg_per_tile = want < max_wg_per_tile ? want : max_wg_per_tile;
  if (wg_per_tile == 0) wg_per_tile = 1;
  if (wg_per_tile > 65535) wg_per_tile = 65535;  // y-dimension limit
  return dim3(tiles, wg_per_tile);
}

extern "C" hipError_t kvc_launch_gather(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, const int32_t* block_ids,
    int num_blocks, const int32_t* ids_dev, uint8_t* dst, hipStream_t stream,
    uint32_t footer_bytes) {
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  const uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  hipLaunchKernelGGL(kvc_gather_blocks, grid, dim3(256), 0, stream,
                     layer_ptrs_dev, layer_strides_dev, num_layers, block_bytes,
                     bl, ids_dev, dst, footer_bytes);
  return hipGetLastError();
}

extern "C" hipError_t kvc_launch_scatter(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, const int32_t* block_ids,
    int num_blocks, const int32_t* ids_dev, const uint8_t* src,
    hipStream_t stream, uint32_t footer_bytes) {
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  const uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  hipLaunchKernelGGL(kvc_scatter_blocks, grid, dim3(256), 0, stream,
                     layer_ptrs_dev, layer_strides_dev, num_layers, block_bytes,
                     bl, ids_dev, src, footer_bytes);
  return hipGetLastError();
}

extern "C" hipError_t kvc_launch_prefix_hash(
    const uint32_t* tokens, const uint64_t* seq_off, const uint64_t* seeds,
    uint64_t* keys, const uint64_t* key_off, int block_size, int n_seq,
    hipStream_t stream) {
  if (n_seq <= 0) return hipSuccess;  // nothing to hash; a 0-wide grid is an error
  int threads = 256;
  int blocks = (n_seq + threads - 1) / threads;
  hipLaunchKernelGGL(kvc_prefix_hash, dim3(blocks), dim3(threads), 0, stream,
                     tokens, seq_off, seeds, keys, key_off, block_size, n_seq);
  return hipGetLastError();
}

}  // namespace kvo

namespace kvo {
// ---- fp8 (OCP e4m3fn) serialization ----------------------------------------
// Fused gather+quantize on store and dequantize+scatter on load: 16-bit KV
// pages (bf16 or fp16, a template parameter — see the page traits below)
// are serialized as fp8 with one f32 scale per (block, layer) tile,
// halving PCIe and storage bytes. Packed slab layout is self-contained per
// tile record (so partial-span tail-seek loads work):
//   [ tile fp8 payload (block_bytes/2) | f32 scale ] x tiles
// gfx950 is OCP e4m3fn (not fnuz). The store side runs split amax+quantize
// passes, the load side a chip-filling sliced dequant — all three grids
// put the tile on blockIdx.x and slices on blockIdx.y like the raw path.

namespace {

// Page formats. Every fp8 kernel below is a template on one of these
// traits: the record layout and all f32 arithmetic are format-free, only
// the page -> f32 conversion on store and the f32 -> page rounding on load
// differ. The launchers pick the trait from their trailing kv_dtype
// argument (kKvBf16 = 0 keeps the bytes this file has always produced).
struct PageBf16 {
  static __device__ __forceinline__ float to_f32(uint16_t u) {
    uint32_t w = static_cast<uint32_t>(u) << 16;
    return __uint_as_float(w);
  }
  static __device__ __forceinline__ uint16_t from_f32(float f) {
    uint32_t w = __float_as_uint(f);
    // round-to-nearest-even
    uint32_t rounding = 0x7fff + ((w >> 16) & 1);
    return static_cast<uint16_t>((w + rounding) >> 16);
  }
};

struct PageFp16 {
  // exact, fp16 subnormals included (v_cvt_f32_f16)
  static __device__ __forceinline__ float to_f32(uint16_t u) {
    return static_cast<float>(__builtin_bit_cast(_Float16, u));
  }
  // Round-to-nearest-even cast that keeps fp16 subnormals; NOT the packed
  // cvt_pkrtz builtin, which rounds toward zero. At the call sites the
  // argument is the product f32(q) * scale. As written here hipcc -O3
  // emits v_pk_mul_f32 + v_cvt_pk_f16_f32 (mode-RNE): the spec's two
  // roundings, f32 then fp16. The compiler is free to fold product and
  // cast into one v_fma_mixlo_f16 instead (it does for the scalar form of
  // this expression, and __fmul_rn does not stop it): a single rounding of
  // the exact product. For every record our encoders write the two agree
  // bit for bit: over all e4m3 codes and every scale = amax/448 with an
  // fp16-representable amax, (m/7) * amax never lies within f32 rounding
  // of an fp16 tie (checked exhaustively on the CPU, 50.4 M pairs), so
  // either form is acceptable and nothing here forces one.
  static __device__ __forceinline__ uint16_t from_f32(float f) {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
  }
};

constexpr int kKvBf16 = 0;
constexpr int kKvFp16 = 1;

// Runs `...` with T bound to the page trait of kv_dtype; an unknown format
// makes the enclosing launcher return hipErrorInvalidValue.
#define KVC_WITH_PAGE_TYPE(kv_dtype, ...)          \
  switch (kv_dtype) {                              \
    case kKvBf16: {                                \
      using T = PageBf16;                          \
      __VA_ARGS__;                                 \
    } break;                                       \
    case kKvFp16: {                                \
      using T = PageFp16;                          \
      __VA_ARGS__;                                 \
    } break;                                       \
    default:                                       \
      return hipErrorInvalidValue;                 \
  }

constexpr float kFp8Max = 448.0f;  // e4m3fn max normal

__device__ __forceinline__ float fp8_e4m3_to_f32(uint8_t b) {
  return __builtin_amdgcn_cvt_f32_fp8(static_cast<uint32_t>(b), 0);
}

}  // namespace

// Pass 1 of the split fp8 gather: per-(tile, wg-slice) partial amax,
// written densely to scratch[tile * gridDim.y + slice] (plain stores — no
// atomics, no zero-init memset, whose fixed ~32 us blit cost ate the
// split's win). Pass 2 reduces the <=slices partials per tile at its
// head. Grid: x = tile, y = slices per tile; both passes use the SAME
// grid.
template <typename T>
__global__ __launch_bounds__(256) void kvc_fp8_amax(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, float* __restrict__ scales) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint16_t* __restrict__ src = reinterpret_cast<const uint16_t*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint4* __restrict__ vsrc = reinterpret_cast<const uint4*>(src);
  const uint64_t nvec = n_elems / 8;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  float amax = 0.0f;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride) {
    uint4 w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      amax = fmaxf(amax, fabsf(T::to_f32(static_cast<uint16_t>(dw[j]))));
      amax = fmaxf(amax, fabsf(T::to_f32(static_cast<uint16_t>(dw[j] >> 16))));
    }
  }
  __shared__ float lds_max[4];
  for (int off = 32; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_down(amax, off, 64));
  if ((threadIdx.x & 63) == 0) lds_max[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = fmaxf(fmaxf(lds_max[0], lds_max[1]), fmaxf(lds_max[2], lds_max[3]));
    scales[static_cast<uint64_t>(tile) * gridDim.y + blockIdx.y] = m;
  }
}

// Pass 2: quantize with full chip parallelism (grid-stride slices per
// tile), reading the tile amax from scales[] and rewriting it as the
// actual scale in the output record.
template <typename T>
__global__ __launch_bounds__(256) void kvc_fp8_quant(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, const float* __restrict__ scales,
    uint8_t* __restrict__ dst, uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint64_t record = n_elems + 4 + footer_bytes;
  const uint16_t* __restrict__ src = reinterpret_cast<const uint16_t*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint4* __restrict__ vsrc = reinterpret_cast<const uint4*>(src);
  uint8_t* __restrict__ payload = dst + static_cast<uint64_t>(tile) * record;
  float amax = 0.0f;
  for (uint32_t g = 0; g < gridDim.y; ++g)
    amax = fmaxf(amax, scales[static_cast<uint64_t>(tile) * gridDim.y + g]);
  if (amax <= 0.0f) amax = 1.0f;
  const float inv_scale = kFp8Max / amax;
  if (blockIdx.y == 0 && threadIdx.x == 0)
    *reinterpret_cast<float*>(payload + n_elems) = amax / kFp8Max;
  uint2* __restrict__ vout = reinterpret_cast<uint2*>(payload);
  const uint64_t nvec = n_elems / 8;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride) {
    uint4 w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
    uint2 out;
    uint32_t lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[0])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[0] >> 16)) * inv_scale, lo, 0);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[1])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[1] >> 16)) * inv_scale, lo, 1);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[2])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[2] >> 16)) * inv_scale, hi, 0);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[3])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[3] >> 16)) * inv_scale, hi, 1);
    out.x = lo;
    out.y = hi;
    vout[v] = out;
  }
}

// Legacy single-workgroup-per-tile fused variant: the zero-copy path keeps
// it (its destination is device-mapped pinned host memory, where the
// split's scratch round trip would cross PCIe).
template <typename T>
__global__ __launch_bounds__(256) void kvc_gather_fp8(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, uint8_t* __restrict__ dst,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;  // 16-bit elements per tile
  const uint64_t record = n_elems + 4 + footer_bytes;  // payload + f32 scale
  const uint16_t* __restrict__ src = reinterpret_cast<const uint16_t*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  uint8_t* __restrict__ payload = dst + static_cast<uint64_t>(tile) * record;
  float* __restrict__ scale_out =
      reinterpret_cast<float*>(payload + n_elems);

  // pass 1: tile amax — 16 B/lane vectorized (8 values per load)
  __shared__ float lds_max[4];
  const uint4* __restrict__ vsrc = reinterpret_cast<const uint4*>(src);
  const uint64_t nvec = n_elems / 8;  // block_bytes % 16 == 0 host-checked
  float amax = 0.0f;
  for (uint64_t v = threadIdx.x; v < nvec; v += blockDim.x) {
    uint4 w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      amax = fmaxf(amax, fabsf(T::to_f32(static_cast<uint16_t>(dw[j]))));
      amax = fmaxf(amax, fabsf(T::to_f32(static_cast<uint16_t>(dw[j] >> 16))));
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_down(amax, off, 64));
  if ((threadIdx.x & 63) == 0) lds_max[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = fmaxf(fmaxf(lds_max[0], lds_max[1]), fmaxf(lds_max[2], lds_max[3]));
    lds_max[0] = m > 0.0f ? m : 1.0f;
    *scale_out = lds_max[0] / kFp8Max;
  }
  __syncthreads();
  const float inv_scale = kFp8Max / lds_max[0];

  // pass 2: quantize — read 8 values, emit 8 fp8 as one dwordx2 store
  uint2* __restrict__ vout = reinterpret_cast<uint2*>(payload);
  for (uint64_t v = threadIdx.x; v < nvec; v += blockDim.x) {
    uint4 w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
    uint2 out;
    uint32_t lo = 0, hi = 0;
    // word_sel must be an immediate: unrolled by hand
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[0])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[0] >> 16)) * inv_scale, lo, 0);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[1])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[1] >> 16)) * inv_scale, lo, 1);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[2])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[2] >> 16)) * inv_scale, hi, 0);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(
        T::to_f32(static_cast<uint16_t>(dw[3])) * inv_scale,
        T::to_f32(static_cast<uint16_t>(dw[3] >> 16)) * inv_scale, hi, 1);
    out.x = lo;
    out.y = hi;
    vout[v] = out;
  }
}

// Chip-filling dequantize+scatter: grid (tile, slices) like the raw path —
// dequant needs no cross-workgroup reduction, the per-tile scale is read
// from the record tail by every slice (uniform L2-hit load). Replaces the
// one-workgroup-per-tile legacy that left the chip 25+% idle on loads.
template <typename T>
__global__ __launch_bounds__(256) void kvc_scatter_fp8(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, const uint8_t* __restrict__ src,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint64_t record = n_elems + 4 + footer_bytes;
  uint16_t* __restrict__ out = reinterpret_cast<uint16_t*>(
      static_cast<uint8_t*>(const_cast<void*>(layer_ptrs[l])) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint8_t* __restrict__ payload =
      src + static_cast<uint64_t>(tile) * record;
  const float scale =
      *reinterpret_cast<const float*>(payload + n_elems);
  // read 8 fp8 as one dwordx2, write 8 page values as one dwordx4
  const uint2* __restrict__ vin = reinterpret_cast<const uint2*>(payload);
  uint4* __restrict__ vout = reinterpret_cast<uint4*>(out);
  const uint64_t nvec = n_elems / 8;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride) {
    uint2 w = vin[v];
    uint4 o;
    uint32_t* od = reinterpret_cast<uint32_t*>(&o);
    const uint32_t words[2] = {w.x, w.y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint8_t b0 = static_cast<uint8_t>(words[j >> 1] >> ((j & 1) * 16));
      uint8_t b1 = static_cast<uint8_t>(words[j >> 1] >> ((j & 1) * 16 + 8));
      uint16_t h0 = T::from_f32(fp8_e4m3_to_f32(b0) * scale);
      uint16_t h1 = T::from_f32(fp8_e4m3_to_f32(b1) * scale);
      od[j] = static_cast<uint32_t>(h0) | (static_cast<uint32_t>(h1) << 16);
    }
    vout[v] = o;
  }
}

extern "C" hipError_t kvc_launch_gather_fp8(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, const int32_t* block_ids,
    int num_blocks, const int32_t* ids_dev, uint8_t* dst, hipStream_t stream,
    uint32_t footer_bytes, int kv_dtype) {
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  int tiles = num_blocks * num_layers;
  KVC_WITH_PAGE_TYPE(
      kv_dtype,
      hipLaunchKernelGGL(kvc_gather_fp8<T>, dim3(tiles), dim3(256), 0, stream,
                         layer_ptrs_dev, layer_strides_dev, num_layers,
                         block_bytes, bl, ids_dev, dst, footer_bytes));
  return hipGetLastError();
}

// Split fp8 gather: amax pass + quantize pass, both chip-filling. scales
// is caller-provided device scratch of `tiles * slices` floats.
extern "C" hipError_t kvc_launch_gather_fp8_split(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, const int32_t* block_ids,
    int num_blocks, const int32_t* ids_dev, uint8_t* dst,
    float* scales_scratch, hipStream_t stream, uint32_t footer_bytes,
    int kv_dtype) {
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  KVC_WITH_PAGE_TYPE(
      kv_dtype,
      hipLaunchKernelGGL(kvc_fp8_amax<T>, grid, dim3(256), 0, stream,
                         layer_ptrs_dev, layer_strides_dev, num_layers,
                         block_bytes, bl, ids_dev, scales_scratch);
      hipLaunchKernelGGL(kvc_fp8_quant<T>, grid, dim3(256), 0, stream,
                         layer_ptrs_dev, layer_strides_dev, num_layers,
                         block_bytes, bl, ids_dev, scales_scratch, dst,
                         footer_bytes));
  return hipGetLastError();
}

extern "C" hipError_t kvc_launch_scatter_fp8(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, const int32_t* block_ids,
    int num_blocks, const int32_t* ids_dev, const uint8_t* src,
    hipStream_t stream, uint32_t footer_bytes, int kv_dtype) {
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  KVC_WITH_PAGE_TYPE(
      kv_dtype,
      hipLaunchKernelGGL(kvc_scatter_fp8<T>, grid, dim3(256), 0, stream,
                         layer_ptrs_dev, layer_strides_dev, num_layers,
                         block_bytes, bl, ids_dev, src, footer_bytes));
  return hipGetLastError();
}

// ---- group-scaled fp8 (one f32 scale per G-element run) ---------------------
// serialize="fp8_e4m3_group": a tile record is
//   [ n fp8 bytes | n/G f32 scales ],  n = block_bytes/2,  n % G == 0
// with G in {64, 128, 256, 512}. At 8 page values per lane a group is G/8 = 8..64
// consecutive lanes of one wave, so the group amax is a log2(G/8)-step xor
// butterfly inside the wave: ONE pass over the source, no scratch slab, no
// LDS, no second launch — which also makes it the right kernel for the
// zero-copy path (nothing but the record itself crosses PCIe).
//
// Per group, all f32: amax = max|x| (0 -> 1), scale = amax/448 (stored),
// q = RNE_e4m3fn(x * (448/amax)); load: y = T_RNE(f32(q) * scale), T the
// page type.

// kLanes = G/8 lanes per group. The grid-stride loop runs on a WAVE-UNIFORM
// base with a guarded body, so every lane of the wave reaches every shuffle
// even when n/8 is not a multiple of 64; groups are kLanes-aligned runs of
// v and n % G == 0, so a group is either wholly inside the tile or wholly
// past its end, and the xor butterfly (offsets < kLanes) never leaves it.
template <int kLanes, typename T>
__global__ __launch_bounds__(256) void kvc_gather_fp8_group(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, uint8_t* __restrict__ dst,
    uint32_t footer_bytes) {
  static_assert(kLanes == 8 || kLanes == 16 || kLanes == 32 || kLanes == 64,
                "group must span 8..64 lanes of one wave");
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint64_t n_groups = n_elems / (8 * kLanes);
  const uint64_t record = n_elems + 4 * n_groups + footer_bytes;
  const uint4* __restrict__ vsrc = reinterpret_cast<const uint4*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  uint8_t* __restrict__ payload = dst + static_cast<uint64_t>(tile) * record;
  uint2* __restrict__ vout = reinterpret_cast<uint2*>(payload);
  float* __restrict__ scales = reinterpret_cast<float*>(payload + n_elems);
  const uint64_t nvec = n_elems / 8;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t vb = static_cast<uint64_t>(blockIdx.y) * blockDim.x +
                     (threadIdx.x & ~63u);
       vb < nvec; vb += stride) {
    const uint64_t v = vb + lane;
    const bool live = v < nvec;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (live) w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
    float x[8];
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = T::to_f32(static_cast<uint16_t>(dw[j]));
      x[2 * j + 1] = T::to_f32(static_cast<uint16_t>(dw[j] >> 16));
      amax = fmaxf(amax, fmaxf(fabsf(x[2 * j]), fabsf(x[2 * j + 1])));
    }
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1)
      amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    if (amax <= 0.0f) amax = 1.0f;
    const float inv_scale = kFp8Max / amax;
    uint2 out;
    uint32_t lo = 0, hi = 0;
    // word_sel must be an immediate: unrolled by hand
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv_scale, x[1] * inv_scale, lo, 0);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv_scale, x[3] * inv_scale, lo, 1);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv_scale, x[5] * inv_scale, hi, 0);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv_scale, x[7] * inv_scale, hi, 1);
    out.x = lo;
    out.y = hi;
    if (live) {
      vout[v] = out;
      if ((lane & (kLanes - 1)) == 0) scales[v / kLanes] = amax / kFp8Max;
    }
  }
}

// Sliced dequantize+scatter for group-scaled records: same shape as
// kvc_scatter_fp8, but the scale is scales[(8 v) / G] = scales[v >> lane_shift]
// (lane_shift = log2(G/8)) — one address per G/8-lane run, an L2-hit load.
template <typename T>
__global__ __launch_bounds__(256) void kvc_scatter_fp8_group(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, int lane_shift, BlockList blocks,
    const int32_t* __restrict__ ids_dev, const uint8_t* __restrict__ src,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint64_t nvec = n_elems / 8;
  const uint64_t record = n_elems + 4 * (nvec >> lane_shift) + footer_bytes;
  uint4* __restrict__ vout = reinterpret_cast<uint4*>(
      static_cast<uint8_t*>(const_cast<void*>(layer_ptrs[l])) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint8_t* __restrict__ payload =
      src + static_cast<uint64_t>(tile) * record;
  const uint2* __restrict__ vin = reinterpret_cast<const uint2*>(payload);
  const float* __restrict__ scales =
      reinterpret_cast<const float*>(payload + n_elems);
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride) {
    const float scale = scales[v >> lane_shift];
    uint2 w = vin[v];
    uint4 o;
    uint32_t* od = reinterpret_cast<uint32_t*>(&o);
    const uint32_t words[2] = {w.x, w.y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint8_t b0 = static_cast<uint8_t>(words[j >> 1] >> ((j & 1) * 16));
      uint8_t b1 = static_cast<uint8_t>(words[j >> 1] >> ((j & 1) * 16 + 8));
      uint16_t h0 = T::from_f32(fp8_e4m3_to_f32(b0) * scale);
      uint16_t h1 = T::from_f32(fp8_e4m3_to_f32(b1) * scale);
      od[j] = static_cast<uint32_t>(h0) | (static_cast<uint32_t>(h1) << 16);
    }
    vout[v] = o;
  }
}

namespace {

// G -> log2(G/8); -1 for anything but 64/128/256/512 or a tile the group
// size does not divide.
inline int fp8_group_lane_shift(uint64_t block_bytes, int group_size) {
  int shift;
  switch (group_size) {
    case 64: shift = 3; break;
    case 128: shift = 4; break;
    case 256: shift = 5; break;
    case 512: shift = 6; break;
    default: return -1;
  }
  if (block_bytes % 16 != 0 ||
      (block_bytes / 2) % static_cast<uint64_t>(group_size) != 0)
    return -1;
  return shift;
}

}  // namespace

extern "C" hipError_t kvc_launch_gather_fp8_group(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, int group_size,
    const int32_t* block_ids, int num_blocks, const int32_t* ids_dev,
    uint8_t* dst, hipStream_t stream, uint32_t footer_bytes, int kv_dtype) {
  const int shift = fp8_group_lane_shift(block_bytes, group_size);
  if (shift < 0) return hipErrorInvalidValue;
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
#define KVC_GATHER_GROUP(LANES)                                             \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kvc_gather_fp8_group<LANES, T>), grid, \
                     dim3(256), 0, stream, layer_ptrs_dev,                  \
                     layer_strides_dev, num_layers, block_bytes, bl,        \
                     ids_dev, dst, footer_bytes)
  KVC_WITH_PAGE_TYPE(
      kv_dtype, switch (shift) {
        case 3: KVC_GATHER_GROUP(8); break;
        case 4: KVC_GATHER_GROUP(16); break;
        case 5: KVC_GATHER_GROUP(32); break;
        default: KVC_GATHER_GROUP(64); break;
      });
#undef KVC_GATHER_GROUP
  return hipGetLastError();
}

extern "C" hipError_t kvc_launch_scatter_fp8_group(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, int group_size,
    const int32_t* block_ids, int num_blocks, const int32_t* ids_dev,
    const uint8_t* src, hipStream_t stream, uint32_t footer_bytes,
    int kv_dtype) {
  const int shift = fp8_group_lane_shift(block_bytes, group_size);
  if (shift < 0) return hipErrorInvalidValue;
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  KVC_WITH_PAGE_TYPE(
      kv_dtype,
      hipLaunchKernelGGL(kvc_scatter_fp8_group<T>, grid, dim3(256), 0, stream,
                         layer_ptrs_dev, layer_strides_dev, num_layers,
                         block_bytes, shift, bl, ids_dev, src, footer_bytes));
  return hipGetLastError();
}

// ---- group-scaled fp4 (OCP e2m1, one f32 scale per G-element run) ------------
// serialize="fp4_e2m1_group": a tile record is
//   [ n/2 code bytes | n/G f32 scales ],  n = block_bytes/2,  n % G == 0
// with G in {16, 32, 64, 128}; element 2i sits in bits 3:0 of byte i, element
// 2i+1 in bits 7:4. The kernels keep the shape of the fp8-group pair: at 8
// page values per lane a group is G/8 = 2..16 consecutive lanes of one wave,
// a lane loads 16 B and stores ONE dword of codes, the group's first lane
// stores the scale.
//
// Per group, all f32: amax = max|x| (0 -> 1), scale = amax/6 (stored),
// t = x * (6/amax), code = sign(x) << 3 | mag(|t|) with mag round-to-nearest-
// even on the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating; load:
// y = T_RNE(f32(value(code)) * scale), T the page type.

namespace {

constexpr float kFp4Max = 6.0f;  // e2m1 max normal

typedef float kvc_float2 __attribute__((ext_vector_type(2)));

// Eight scaled values -> one dword of codes, element j in bits 4j+3:4j, with
// the gfx950 packed convert (v_cvt_scalef32_pk_fp4_f32 at scale 1.0: two
// values per instruction, into the selected byte). The format is defined by
// the compare chain of the host twin (engine.h f32_to_fp4_rne: RNE, ties to
// the even code, saturating at 6, the sign bit always copied, so -0.0 and
// negatives that round to zero give 0x8); the instruction returned the
// chain's code for every finite f32 bit pattern when the two were compared
// exhaustively on an MI355X, and the tests hold both to the oracle's bytes.
// A compare chain here costs ~17 VALU instructions per value and made the
// gather compute-bound (profiles/fp4_group_kernels.md).
__device__ __forceinline__ uint32_t fp4_e2m1_pack8(const float (&t)[8]) {
  uint32_t out = 0;
  // byte_sel must be an immediate: unrolled by hand
  out = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(out, t[0], t[1], 1.0f, 0);
  out = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(out, t[2], t[3], 1.0f, 1);
  out = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(out, t[4], t[5], 1.0f, 2);
  out = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(out, t[6], t[7], 1.0f, 3);
  return out;
}

// Byte kByte of a code dword -> its two values (low nibble first); exact, no
// rounding is involved (v_cvt_scalef32_pk_f32_fp4 at scale 1.0).
template <int kByte>
__device__ __forceinline__ kvc_float2 fp4_e2m1_unpack2(uint32_t codes) {
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(codes, 1.0f, kByte);
}

// Page value of an f32 product that has ALREADY been rounded to f32: the
// second of the spec's two roundings. Unlike the fp8 records (see
// PageFp16::from_f32), fp4 records do hit fp16 ties where one rounding of
// the exact product and two roundings differ (magnitudes 1.5 and 3.0 times
// a scale amax/6, subnormal results), so the fp16 form must not let the
// compiler fold product and cast into one mixed-precision FMA: the empty
// asm makes the f32 product opaque, and the cast that follows is a plain
// v_cvt_f16_f32 (RNE, fp16 subnormals kept). bf16 rounds in integer
// arithmetic on the f32 bits and cannot be folded.
template <typename T>
__device__ __forceinline__ uint16_t fp4_page_from_product(float p) {
  return T::from_f32(p);
}
template <>
__device__ __forceinline__ uint16_t fp4_page_from_product<PageFp16>(float p) {
  asm("" : "+v"(p));
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(p));
}

}  // namespace

// kLanes = G/8 lanes per group. Same loop as kvc_gather_fp8_group: a
// WAVE-UNIFORM grid-stride base with a guarded body, so every lane reaches
// every shuffle; groups are kLanes-aligned runs of v and n % G == 0, so a
// group is wholly inside the tile or wholly past its end, and the xor
// butterfly (offsets < kLanes) never leaves it.
template <int kLanes, typename T>
__global__ __launch_bounds__(256) void kvc_gather_fp4_group(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, uint8_t* __restrict__ dst,
    uint32_t footer_bytes) {
  static_assert(kLanes == 2 || kLanes == 4 || kLanes == 8 || kLanes == 16,
                "group must span 2..16 lanes of one wave");
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint64_t n_groups = n_elems / (8 * kLanes);
  const uint64_t record = n_elems / 2 + 4 * n_groups + footer_bytes;
  const uint4* __restrict__ vsrc = reinterpret_cast<const uint4*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  uint8_t* __restrict__ payload = dst + static_cast<uint64_t>(tile) * record;
  uint32_t* __restrict__ vout = reinterpret_cast<uint32_t*>(payload);
  float* __restrict__ scales = reinterpret_cast<float*>(payload + n_elems / 2);
  const uint64_t nvec = n_elems / 8;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t vb = static_cast<uint64_t>(blockIdx.y) * blockDim.x +
                     (threadIdx.x & ~63u);
       vb < nvec; vb += stride) {
    const uint64_t v = vb + lane;
    const bool live = v < nvec;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (live) w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
    float x[8];
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = T::to_f32(static_cast<uint16_t>(dw[j]));
      x[2 * j + 1] = T::to_f32(static_cast<uint16_t>(dw[j] >> 16));
      amax = fmaxf(amax, fmaxf(fabsf(x[2 * j]), fabsf(x[2 * j + 1])));
    }
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1)
      amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    if (amax <= 0.0f) amax = 1.0f;
    const float inv_scale = kFp4Max / amax;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] *= inv_scale;
    const uint32_t out = fp4_e2m1_pack8(x);
    if (live) {
      vout[v] = out;
      if ((lane & (kLanes - 1)) == 0) scales[v / kLanes] = amax / kFp4Max;
    }
  }
}

// Sliced dequantize+scatter for fp4 records: the shape of
// kvc_scatter_fp8_group. A lane reads one dword of codes and writes 8 page
// values as one dwordx4; its scale is scales[(8 v) / G] = scales[v >>
// lane_shift] (lane_shift = log2(G/8)), one address per G/8-lane run.
template <typename T>
__global__ __launch_bounds__(256) void kvc_scatter_fp4_group(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, int lane_shift, BlockList blocks,
    const int32_t* __restrict__ ids_dev, const uint8_t* __restrict__ src,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes / 2;
  const uint64_t nvec = n_elems / 8;
  const uint64_t record = n_elems / 2 + 4 * (nvec >> lane_shift) + footer_bytes;
  uint4* __restrict__ vout = reinterpret_cast<uint4*>(
      static_cast<uint8_t*>(const_cast<void*>(layer_ptrs[l])) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint8_t* __restrict__ payload =
      src + static_cast<uint64_t>(tile) * record;
  const uint32_t* __restrict__ vin = reinterpret_cast<const uint32_t*>(payload);
  const float* __restrict__ scales =
      reinterpret_cast<const float*>(payload + n_elems / 2);
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride) {
    const float scale = scales[v >> lane_shift];
    const uint32_t codes = vin[v];
    // byte_sel must be an immediate: unrolled by hand
    const kvc_float2 val[4] = {
        fp4_e2m1_unpack2<0>(codes), fp4_e2m1_unpack2<1>(codes),
        fp4_e2m1_unpack2<2>(codes), fp4_e2m1_unpack2<3>(codes)};
    uint4 o;
    uint32_t* od = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint16_t h0 = fp4_page_from_product<T>(val[j].x * scale);
      uint16_t h1 = fp4_page_from_product<T>(val[j].y * scale);
      od[j] = static_cast<uint32_t>(h0) | (static_cast<uint32_t>(h1) << 16);
    }
    vout[v] = o;
  }
}

// ---- fp4 records over fp8 (OCP e4m3fn) pages ---------------------------------
// kv_dtype="float8_e4m3fn": the page already is one byte per element, so a
// tile holds n = block_bytes elements (not block_bytes/2) and the record is
//   [ n/2 code bytes | n/G f32 scales ],  n % G == 0,  G in {16, 32, 64, 128}.
// The arithmetic is the fp4 spec above with x = the exact f32 value of the
// page byte and the load rounding to e4m3fn: y = RNE_e4m3fn(f32(value(code))
// * scale), subnormals kept, the sign copied even when the magnitude rounds
// to zero (-0.0 and negatives that underflow load as 0x80). NaN page bytes
// (0x7f/0xff) are out of scope.
//
// 16 page values per lane: a lane loads 16 B, stores 8 B of codes, and a
// group is G/16 = 1..8 consecutive lanes (0..3 butterfly steps).
// copy_grid(tiles, block_bytes) yields exactly block_bytes/16 vectors per
// tile. Records are multiples of 4 bytes but not of 8 (G=32 at 32-byte
// tiles: 20 bytes), so the 8-byte code accesses land at 4 mod 8, like the
// per-tile fp8 kernels' stores.

namespace {

constexpr int kKvFp8E4M3 = 2;

// One dword of page bytes -> its four exact f32 values (v_cvt_pk_f32_fp8).
__device__ __forceinline__ void fp8_page_unpack4(uint32_t w, float* x) {
  const kvc_float2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  const kvc_float2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  x[0] = lo.x;
  x[1] = lo.y;
  x[2] = hi.x;
  x[3] = hi.y;
}

// Four f32 products (already rounded to f32) -> one dword of page bytes:
// v_cvt_pk_fp8_f32, RNE with e4m3 subnormals. The instruction keeps the
// sign of -0.0 and of a negative that underflows (0x80), which is what the
// format asks for (measured on an MI355X against the host twin over every
// value(code) * scale our encoders can write; profiles/
// fp8_page_fp4_kernels.md), so no fix-up follows it.
__device__ __forceinline__ uint32_t fp8_page_pack4(float p0, float p1, float p2,
                                                   float p3) {
  uint32_t w = 0;
  // word_sel must be an immediate: unrolled by hand
  w = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, w, true);
  return w;
}

}  // namespace

// kLanes = G/16 lanes per group. Same loop as kvc_gather_fp4_group: a
// WAVE-UNIFORM grid-stride base with a guarded body, so every lane reaches
// every shuffle; groups are kLanes-aligned runs of v and n % G == 0, so a
// group is wholly inside the tile or wholly past its end, and the xor
// butterfly (offsets < kLanes) never leaves it.
template <int kLanes>
__global__ __launch_bounds__(256) void kvc_gather_fp4_group_fp8page(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, BlockList blocks,
    const int32_t* __restrict__ ids_dev, uint8_t* __restrict__ dst,
    uint32_t footer_bytes) {
  static_assert(kLanes == 1 || kLanes == 2 || kLanes == 4 || kLanes == 8,
                "group must span 1..8 lanes of one wave");
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes;  // one byte per page element
  const uint64_t n_groups = n_elems / (16 * kLanes);
  const uint64_t record = n_elems / 2 + 4 * n_groups + footer_bytes;
  const uint4* __restrict__ vsrc = reinterpret_cast<const uint4*>(
      static_cast<const uint8_t*>(layer_ptrs[l]) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  uint8_t* __restrict__ payload = dst + static_cast<uint64_t>(tile) * record;
  uint2* __restrict__ vout = reinterpret_cast<uint2*>(payload);
  float* __restrict__ scales = reinterpret_cast<float*>(payload + n_elems / 2);
  const uint64_t nvec = n_elems / 16;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t vb = static_cast<uint64_t>(blockIdx.y) * blockDim.x +
                     (threadIdx.x & ~63u);
       vb < nvec; vb += stride) {
    const uint64_t v = vb + lane;
    const bool live = v < nvec;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (live) w = vsrc[v];
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&w);
    float x[16];
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fp8_page_unpack4(dw[j], x + 4 * j);
      amax = fmaxf(fmaxf(amax, fmaxf(fabsf(x[4 * j]), fabsf(x[4 * j + 1]))),
                   fmaxf(fabsf(x[4 * j + 2]), fabsf(x[4 * j + 3])));
    }
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1)
      amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    if (amax <= 0.0f) amax = 1.0f;
    const float inv_scale = kFp4Max / amax;
    float lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lo[j] = x[j] * inv_scale;
      hi[j] = x[8 + j] * inv_scale;
    }
    uint2 out;
    out.x = fp4_e2m1_pack8(lo);
    out.y = fp4_e2m1_pack8(hi);
    if (live) {
      vout[v] = out;
      if ((lane & (kLanes - 1)) == 0) scales[v / kLanes] = amax / kFp4Max;
    }
  }
}

// Sliced dequantize+scatter of fp4 records into fp8 pages: the shape of
// kvc_scatter_fp4_group at 16 values per lane. A lane reads 8 B of codes and
// writes 16 page bytes as one dwordx4; its scale is scales[(16 v) / G] =
// scales[v >> lane_shift] (lane_shift = log2(G/16)).
__global__ __launch_bounds__(256) void kvc_scatter_fp4_group_fp8page(
    const void* const* __restrict__ layer_ptrs,
    const uint64_t* __restrict__ layer_strides, int num_layers,
    uint64_t block_bytes, int lane_shift, BlockList blocks,
    const int32_t* __restrict__ ids_dev, const uint8_t* __restrict__ src,
    uint32_t footer_bytes) {
  const uint32_t tile = blockIdx.x;
  const int l = tile % num_layers;
  const int bi = tile / num_layers;
  const uint64_t n_elems = block_bytes;
  const uint64_t nvec = n_elems / 16;
  const uint64_t record = n_elems / 2 + 4 * (nvec >> lane_shift) + footer_bytes;
  uint4* __restrict__ vout = reinterpret_cast<uint4*>(
      static_cast<uint8_t*>(const_cast<void*>(layer_ptrs[l])) +
      static_cast<uint64_t>(block_id(blocks, ids_dev, bi)) * layer_strides[l]);
  const uint8_t* __restrict__ payload =
      src + static_cast<uint64_t>(tile) * record;
  const uint2* __restrict__ vin = reinterpret_cast<const uint2*>(payload);
  const float* __restrict__ scales =
      reinterpret_cast<const float*>(payload + n_elems / 2);
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * blockDim.x;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.y) * blockDim.x + threadIdx.x;
       v < nvec; v += stride) {
    const float scale = scales[v >> lane_shift];
    const uint2 codes = vin[v];
    // byte_sel must be an immediate: unrolled by hand
    const kvc_float2 val[8] = {
        fp4_e2m1_unpack2<0>(codes.x), fp4_e2m1_unpack2<1>(codes.x),
        fp4_e2m1_unpack2<2>(codes.x), fp4_e2m1_unpack2<3>(codes.x),
        fp4_e2m1_unpack2<0>(codes.y), fp4_e2m1_unpack2<1>(codes.y),
        fp4_e2m1_unpack2<2>(codes.y), fp4_e2m1_unpack2<3>(codes.y)};
    uint4 o;
    uint32_t* od = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      od[j] = fp8_page_pack4(val[2 * j].x * scale, val[2 * j].y * scale,
                             val[2 * j + 1].x * scale, val[2 * j + 1].y * scale);
    vout[v] = o;
  }
}

namespace {

// G -> log2(G / values per lane), 8 values per lane for 16-bit pages and 16
// for fp8 pages; -1 for anything but 16/32/64/128, a page format the fp4
// kernels do not read, or a tile the group size does not divide.
inline int fp4_group_lane_shift(uint64_t block_bytes, int group_size,
                                int kv_dtype) {
  int shift;
  switch (group_size) {
    case 16: shift = 1; break;
    case 32: shift = 2; break;
    case 64: shift = 3; break;
    case 128: shift = 4; break;
    default: return -1;
  }
  if (block_bytes % 16 != 0) return -1;
  uint64_t n_elems;
  if (kv_dtype == kKvFp8E4M3) {
    n_elems = block_bytes;
    shift -= 1;
  } else if (kv_dtype == kKvBf16 || kv_dtype == kKvFp16) {
    n_elems = block_bytes / 2;
  } else {
    return -1;
  }
  if (n_elems % static_cast<uint64_t>(group_size) != 0) return -1;
  return shift;
}

}  // namespace

extern "C" hipError_t kvc_launch_gather_fp4_group(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, int group_size,
    const int32_t* block_ids, int num_blocks, const int32_t* ids_dev,
    uint8_t* dst, hipStream_t stream, uint32_t footer_bytes, int kv_dtype) {
  const int shift = fp4_group_lane_shift(block_bytes, group_size, kv_dtype);
  if (shift < 0) return hipErrorInvalidValue;
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  if (kv_dtype == kKvFp8E4M3) {
#define KVC_GATHER_FP4_FP8PAGE(LANES)                                        \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kvc_gather_fp4_group_fp8page<LANES>),   \
                     grid, dim3(256), 0, stream, layer_ptrs_dev,             \
                     layer_strides_dev, num_layers, block_bytes, bl,         \
                     ids_dev, dst, footer_bytes)
    switch (shift) {
      case 0: KVC_GATHER_FP4_FP8PAGE(1); break;
      case 1: KVC_GATHER_FP4_FP8PAGE(2); break;
      case 2: KVC_GATHER_FP4_FP8PAGE(4); break;
      default: KVC_GATHER_FP4_FP8PAGE(8); break;
    }
#undef KVC_GATHER_FP4_FP8PAGE
    return hipGetLastError();
  }
#define KVC_GATHER_FP4_GROUP(LANES)                                         \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(kvc_gather_fp4_group<LANES, T>), grid, \
                     dim3(256), 0, stream, layer_ptrs_dev,                  \
                     layer_strides_dev, num_layers, block_bytes, bl,        \
                     ids_dev, dst, footer_bytes)
  KVC_WITH_PAGE_TYPE(
      kv_dtype, switch (shift) {
        case 1: KVC_GATHER_FP4_GROUP(2); break;
        case 2: KVC_GATHER_FP4_GROUP(4); break;
        case 3: KVC_GATHER_FP4_GROUP(8); break;
        default: KVC_GATHER_FP4_GROUP(16); break;
      });
#undef KVC_GATHER_FP4_GROUP
  return hipGetLastError();
}

extern "C" hipError_t kvc_launch_scatter_fp4_group(
    const void* const* layer_ptrs_dev, const uint64_t* layer_strides_dev,
    int num_layers, uint64_t block_bytes, int group_size,
    const int32_t* block_ids, int num_blocks, const int32_t* ids_dev,
    const uint8_t* src, hipStream_t stream, uint32_t footer_bytes,
    int kv_dtype) {
  const int shift = fp4_group_lane_shift(block_bytes, group_size, kv_dtype);
  if (shift < 0) return hipErrorInvalidValue;
  BlockList bl;
  if (ids_dev == nullptr) {
    if (num_blocks > kMaxBlocksPerFile) return hipErrorInvalidValue;
    for (int i = 0; i < num_blocks; ++i) bl.ids[i] = block_ids[i];
  }
  uint32_t tiles = static_cast<uint32_t>(num_blocks) * num_layers;
  dim3 grid = copy_grid(tiles, block_bytes);
  if (kv_dtype == kKvFp8E4M3) {
    hipLaunchKernelGGL(kvc_scatter_fp4_group_fp8page, grid, dim3(256), 0,
                       stream, layer_ptrs_dev, layer_strides_dev, num_layers,
                       block_bytes, shift, bl, ids_dev, src, footer_bytes);
    return hipGetLastError();
  }
  KVC_WITH_PAGE_TYPE(
      kv_dtype,
      hipLaunchKernelGGL(kvc_scatter_fp4_group<T>, grid, dim3(256), 0, stream,
                         layer_ptrs_dev, layer_strides_dev, num_layers,
                         block_bytes, shift, bl, ids_dev, src, footer_bytes));
  return hipGetLastError();
}


// ---- per-record checksums ----------------------------------------------------
// EngineConfig::checksum appends a 16-byte footer to every tile record:
//   [ payload (P bytes, P % 4 == 0) | sum u64 | magic "KVCS" | P as u32 ]
// sum = SUM_i mix(((i + 1) << 32) | w[i]) mod 2^64 over the payload's u32
// words, mix = the splitmix64 finalizer (checksum.h is the host twin and
// must produce the same bytes). Addition commutes, so partial sums combine
// in any order:
//   pass 1 (kvc_record_partial_sums): grid (tile, slices) as the copy
//     kernels; lane -> wave shuffle -> LDS -> one plain 64-bit store per
//     workgroup to partials[tile * slices + slice] (no atomics, no memset —
//     see kvc_fp8_amax for what a zero-init blit costs);
//   pass 2 (kvc_seal_records / kvc_verify_records): adds the <= slices
//     partials of a tile and writes, or compares, the footer.
// fp8 records are only 4-byte aligned (stride n + 20), so pass 1 peels up to
// three leading words to reach a 16-byte boundary, reads the body as
// dwordx4 and picks up the <= 3 trailing words; the footer is written and
// read as four dwords, never as one 8-byte access.

namespace {

constexpr uint32_t kCsumMagic = 0x5343564Bu;
constexpr uint32_t kCsumFooterBytes = 16;

__device__ __forceinline__ uint64_t csum_mix(uint64_t index, uint32_t word) {
  uint64_t x = ((index + 1) << 32) | word;
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

}  // namespace

__global__ __launch_bounds__(256) void kvc_record_partial_sums(
    const uint8_t* __restrict__ slab, uint32_t payload_bytes,
    uint64_t* __restrict__ partials) {
  const uint32_t tile = blockIdx.x;
  const uint8_t* __restrict__ rec =
      slab + static_cast<uint64_t>(tile) * (payload_bytes + kCsumFooterBytes);
  const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(rec);
  const uint32_t nwords = payload_bytes / 4;
  uint32_t head =
      static_cast<uint32_t>((16 - (reinterpret_cast<uintptr_t>(rec) & 15)) & 15) / 4;
  if (head > nwords) head = nwords;
  const uint32_t nvec = (nwords - head) / 4;
  const uint32_t tail = nwords - head - nvec * 4;
  const uint4* __restrict__ body = reinterpret_cast<const uint4*>(words + head);
  uint64_t acc = 0;
  const uint32_t stride = gridDim.y * blockDim.x;
  for (uint32_t v = blockIdx.y * blockDim.x + threadIdx.x; v < nvec;
       v += stride) {
    const uint4 w = body[v];
    const uint64_t i = head + 4ull * v;
    acc += csum_mix(i, w.x) + csum_mix(i + 1, w.y) + csum_mix(i + 2, w.z) +
           csum_mix(i + 3, w.w);
  }
  // the <= 3 head and <= 3 tail words ride the first lanes of slice 0
  if (blockIdx.y == 0 && threadIdx.x < head + tail) {
    const uint32_t i = threadIdx.x < head
                           ? threadIdx.x
                           : head + nvec * 4 + (threadIdx.x - head);
    acc += csum_mix(i, words[i]);
  }
  __shared__ uint64_t lds_sum[4];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) lds_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[static_cast<uint64_t>(tile) * gridDim.y + blockIdx.y] =
        lds_sum[0] + lds_sum[1] + lds_sum[2] + lds_sum[3];
}

// One lane per record: writes the whole footer, whatever it held before.
__global__ __launch_bounds__(256) void kvc_seal_records(
    uint8_t* __restrict__ slab, uint32_t tiles, uint32_t payload_bytes,
    const uint64_t* __restrict__ partials, uint32_t slices) {
  const uint32_t tile = blockIdx.x * blockDim.x + threadIdx.x;
  if (tile >= tiles) return;
  uint64_t sum = 0;
  for (uint32_t g = 0; g < slices; ++g)
    sum += partials[static_cast<uint64_t>(tile) * slices + g];
  uint32_t* __restrict__ footer = reinterpret_cast<uint32_t*>(
      slab + static_cast<uint64_t>(tile) * (payload_bytes + kCsumFooterBytes) +
      payload_bytes);
  footer[0] = static_cast<uint32_t>(sum);
  footer[1] = static_cast<uint32_t>(sum >> 32);
  footer[2] = kCsumMagic;
  footer[3] = payload_bytes;
}

// One workgroup walks every record and leaves result[0] = number of records
// whose footer does not match, result[1] = index of the first one
// (0xffffffff when none). Read-only on the slab; result needs no zero-init.
__global__ __launch_bounds__(256) void kvc_verify_records(
    const uint8_t* __restrict__ slab, uint32_t tiles, uint32_t payload_bytes,
    const uint64_t* __restrict__ partials, uint32_t slices,
    uint32_t* __restrict__ result) {
  uint32_t bad = 0, first = 0xffffffffu;
  for (uint32_t tile = threadIdx.x; tile < tiles; tile += blockDim.x) {
    uint64_t sum = 0;
    for (uint32_t g = 0; g < slices; ++g)
      sum += partials[static_cast<uint64_t>(tile) * slices + g];
    const uint32_t* __restrict__ footer = reinterpret_cast<const uint32_t*>(
        slab + static_cast<uint64_t>(tile) * (payload_bytes + kCsumFooterBytes) +
        payload_bytes);
    const bool ok = footer[0] == static_cast<uint32_t>(sum) &&
                    footer[1] == static_cast<uint32_t>(sum >> 32) &&
                    footer[2] == kCsumMagic && footer[3] == payload_bytes;
    if (!ok) {
      ++bad;
      first = first < tile ? first : tile;
    }
  }
  __shared__ uint32_t lds_bad[4], lds_first[4];
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_down(bad, off, 64);
    const uint32_t other = __shfl_down(first, off, 64);
    first = first < other ? first : other;
  }
  if ((threadIdx.x & 63) == 0) {
    lds_bad[threadIdx.x >> 6] = bad;
    lds_first[threadIdx.x >> 6] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t f = lds_first[0];
    for (int w = 1; w < 4; ++w) f = f < lds_first[w] ? f : lds_first[w];
    result[0] = lds_bad[0] + lds_bad[1] + lds_bad[2] + lds_bad[3];
    result[1] = f;
  }
}

// Scratch the two checksum launchers need: one u64 per (tile, slice), and
// copy_grid never makes more than tiles + 2048 workgroups.
extern "C" size_t kvc_checksum_scratch_bytes(size_t tiles) {
  return (tiles + 2048) * sizeof(uint64_t);
}

namespace {

inline bool csum_args_ok(const void* slab, uint32_t tiles,
                         uint64_t payload_bytes, const void* scratch) {
  return tiles > 0 && payload_bytes > 0 && payload_bytes % 4 == 0 &&
         payload_bytes <= 0xfffffff0ull &&
         (reinterpret_cast<uintptr_t>(slab) & 3) == 0 &&
         (reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && scratch != nullptr;
}

}  // namespace

// slab: `tiles` records of payload_bytes + 16, 4-byte aligned; scratch:
// kvc_checksum_scratch_bytes(tiles) of 8-byte aligned device memory.
extern "C" hipError_t kvc_launch_seal_records(uint8_t* slab, uint32_t tiles,
                                              uint64_t payload_bytes,
                                              uint64_t* scratch,
                                              hipStream_t stream) {
  if (!csum_args_ok(slab, tiles, payload_bytes, scratch))
    return hipErrorInvalidValue;
  const uint32_t pb = static_cast<uint32_t>(payload_bytes);
  dim3 grid = copy_grid(tiles, payload_bytes);
  hipLaunchKernelGGL(kvc_record_partial_sums, grid, dim3(256), 0, stream, slab,
                     pb, scratch);
  hipLaunchKernelGGL(kvc_seal_records, dim3((tiles + 255) / 256), dim3(256), 0,
                     stream, slab, tiles, pb, scratch, grid.y);
  return hipGetLastError();
}

// result: two u32 the device can write (bad count, first bad index).
extern "C" hipError_t kvc_launch_verify_records(const uint8_t* slab,
                                                uint32_t tiles,
                                                uint64_t payload_bytes,
                                                uint64_t* scratch,
                                                uint32_t* result,
                                                hipStream_t stream) {
  if (!csum_args_ok(slab, tiles, payload_bytes, scratch) || result == nullptr)
    return hipErrorInvalidValue;
  const uint32_t pb = static_cast<uint32_t>(payload_bytes);
  dim3 grid = copy_grid(tiles, payload_bytes);
  hipLaunchKernelGGL(kvc_record_partial_sums, grid, dim3(256), 0, stream, slab,
                     pb, scratch);
  hipLaunchKernelGGL(kvc_verify_records, dim3(1), dim3(256), 0, stream, slab,
                     tiles, pb, scratch, grid.y, result);
  return hipGetLastError();
}

}  // namespace kvo
