// BlockCopier: standalone gather/scatter between paged KV tensors and a
// contiguous buffer — the packing primitive of the xGMI peer-migration
// path (peer rank gathers blocks into a send slab, RCCL ships it, the
// puller scatters into its own pages). Same kernels as the offload engine;
// host mode memcpys for CPU-only tests.
//
// Every packed_bytes*/gather*/scatter* call takes checksum=false|true: true
// selects the record stride payload + 16 (checksum.h) and leaves the footer
// bytes alone; seal_records() then fills the footers of any such slab and
// verify_records() checks them.
//
// kv_dtype (bf16 by default) is the format of the pages; every fp8 and fp4
// method of the copier converts with it, the raw ones never look at it. A
// copier over fp8 (e4m3fn) pages has the raw and the fp4 methods only: its
// *_fp8 and *_fp8_group methods throw, the pages already are fp8.
#pragma once

#include <mutex>
#include <utility>

#include "checksum.h"
#include "common.h"
#include "engine.h"  // GroupDesc, kernel launcher decls

namespace kvo {

class BlockCopier {
 public:
  BlockCopier(std::vector<GroupDesc> groups, bool gpu_mode, int device,
              KvDtype kv_dtype = KvDtype::kBf16)
      : groups_(std::move(groups)), gpu_mode_(gpu_mode), kv_dtype_(kv_dtype) {
    if (gpu_mode_) {
      KVO_HIP_CHECK(hipSetDevice(device));
      for (auto& g : groups_) {
        void* dp = nullptr;
        KVO_HIP_CHECK(hipMalloc(&dp, g.layer_ptrs.size() * sizeof(void*)));
        KVO_HIP_CHECK(hipMemcpy(dp, g.layer_ptrs.data(),
                                g.layer_ptrs.size() * sizeof(void*),
                                hipMemcpyHostToDevice));
        dev_layer_ptrs_.push_back(static_cast<void**>(dp));
        void* ds = nullptr;
        KVO_HIP_CHECK(hipMalloc(&ds, g.layer_strides.size() * sizeof(uint64_t)));
        KVO_HIP_CHECK(hipMemcpy(ds, g.layer_strides.data(),
                                g.layer_strides.size() * sizeof(uint64_t),
                                hipMemcpyHostToDevice));
        dev_layer_strides_.push_back(static_cast<uint64_t*>(ds));
      }
    }
  }

  ~BlockCopier() {
    for (auto p : dev_layer_ptrs_) (void)hipFree(p);
    for (auto p : dev_layer_strides_) (void)hipFree(p);
    if (csum_scratch_) (void)hipFree(csum_scratch_);
  }

  size_t packed_bytes(int group, size_t n_blocks, bool checksum = false) const {
    const GroupDesc& g = groups_.at(group);
    return n_blocks * g.layer_ptrs.size() * (g.block_bytes + footer(checksum));
  }

  // fp8 e4m3 record size: block_bytes/2 payload + f32 scale per tile.
  size_t packed_bytes_fp8(int group, size_t n_blocks,
                          bool checksum = false) const {
    check_not_fp8_pages();
    const GroupDesc& g = groups_.at(group);
    return n_blocks * g.layer_ptrs.size() *
           (g.block_bytes / 2 + 4 + footer(checksum));
  }

  // Fill the checksum footer of every record of a slab of `tiles` records
  // of payload_bytes + 16 (device ptr in GPU mode, async on `stream`),
  // whatever the footers held before. GPU-mode calls of one copier share
  // one scratch slab: keep them on one stream, or synchronize in between.
  void seal_records(void* slab, size_t tiles, size_t payload_bytes,
                    uintptr_t stream) {
    check_records(slab, tiles, payload_bytes);
    if (!gpu_mode_) {
      seal_records_host(static_cast<uint8_t*>(slab), tiles, payload_bytes);
      return;
    }
    std::lock_guard<std::mutex> g(csum_mu_);
    ensure_csum_buffers(tiles);
    hipError_t err = kvc_launch_seal_records(
        static_cast<uint8_t*>(slab), static_cast<uint32_t>(tiles),
        payload_bytes, csum_scratch_, reinterpret_cast<hipStream_t>(stream));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Check every footer of such a slab. Returns (bad records, index of the
  // first bad one or -1); read-only on the slab. Synchronizes `stream` in
  // GPU mode.
  std::pair<int64_t, int64_t> verify_records(const void* slab, size_t tiles,
                                             size_t payload_bytes,
                                             uintptr_t stream) {
    check_records(slab, tiles, payload_bytes);
    if (!gpu_mode_) {
      int64_t first = -1;
      size_t bad = verify_records_host(static_cast<const uint8_t*>(slab), tiles,
                                       payload_bytes, &first);
      return {static_cast<int64_t>(bad), first};
    }
    std::lock_guard<std::mutex> g(csum_mu_);
    ensure_csum_buffers(tiles);
    volatile uint32_t* res =
        reinterpret_cast<volatile uint32_t*>(csum_result_->host());
    hipError_t err = kvc_launch_verify_records(
        static_cast<const uint8_t*>(slab), static_cast<uint32_t>(tiles),
        payload_bytes, csum_scratch_,
        reinterpret_cast<uint32_t*>(csum_result_->device()),
        reinterpret_cast<hipStream_t>(stream));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
    KVO_HIP_CHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    const uint32_t bad = res[0], first = res[1];
    return {static_cast<int64_t>(bad),
            bad == 0 ? -1 : static_cast<int64_t>(first)};
  }

  // Scratch floats the fp8 gather needs beyond the packed output
  // (partial-max slab; copy_grid caps slices at 2048/tiles + 1).
  size_t fp8_scratch_bytes(int group, size_t n_blocks) const {
    const GroupDesc& g = groups_.at(group);
    size_t tiles = n_blocks * g.layer_ptrs.size();
    return (tiles + 4096) * sizeof(float);
  }

  // Gather + quantize into dst (device ptr, GPU mode); scratch must hold
  // fp8_scratch_bytes(). Host mode uses the software codec.
  void gather_fp8(int group, const std::vector<int32_t>& ids, void* dst,
                  void* scratch, uintptr_t stream, bool checksum = false) {
    check_not_fp8_pages();
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    if (!gpu_mode_) {
      host_fp8(g, ids, static_cast<uint8_t*>(dst), /*quantize=*/true,
               footer(checksum));
      return;
    }
    hipError_t err = kvc_launch_gather_fp8_split(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, ids.data(), static_cast<int>(ids.size()), nullptr,
        static_cast<uint8_t*>(dst), static_cast<float*>(scratch),
        reinterpret_cast<hipStream_t>(stream), footer(checksum),
        static_cast<int>(kv_dtype_));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Dequantize + scatter from an fp8 record slab.
  void scatter_fp8(int group, const std::vector<int32_t>& ids, const void* src,
                   uintptr_t stream, bool checksum = false) {
    check_not_fp8_pages();
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    if (!gpu_mode_) {
      host_fp8(g, ids,
               const_cast<uint8_t*>(static_cast<const uint8_t*>(src)),
               /*quantize=*/false, footer(checksum));
      return;
    }
    hipError_t err = kvc_launch_scatter_fp8(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, ids.data(), static_cast<int>(ids.size()), nullptr,
        static_cast<const uint8_t*>(src), reinterpret_cast<hipStream_t>(stream),
        footer(checksum), static_cast<int>(kv_dtype_));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Group-scaled fp8 record size: block_bytes/2 payload + one f32 scale
  // per group_size elements, per tile.
  size_t packed_bytes_fp8_group(int group, size_t n_blocks, int group_size,
                                bool checksum = false) const {
    check_not_fp8_pages();
    const GroupDesc& g = groups_.at(group);
    check_group_size(g, group_size);
    return n_blocks * g.layer_ptrs.size() *
           (StorageOffloadEngine::fp8_group_record_bytes(g.block_bytes,
                                                         group_size) +
            footer(checksum));
  }

  // Single-pass gather + per-group quantize into dst (device ptr in GPU
  // mode); needs no scratch. Host mode uses the software twin.
  void gather_fp8_group(int group, const std::vector<int32_t>& ids, void* dst,
                        int group_size, uintptr_t stream,
                        bool checksum = false) {
    check_not_fp8_pages();
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    check_group_size(g, group_size);
    if (!gpu_mode_) {
      StorageOffloadEngine::host_fp8_group_copy(
          g, ids, static_cast<uint8_t*>(dst), group_size, /*quantize=*/true,
          footer(checksum), kv_dtype_);
      return;
    }
    hipError_t err = kvc_launch_gather_fp8_group(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, group_size, ids.data(), static_cast<int>(ids.size()),
        nullptr, static_cast<uint8_t*>(dst),
        reinterpret_cast<hipStream_t>(stream), footer(checksum),
        static_cast<int>(kv_dtype_));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Dequantize + scatter from a group-scaled fp8 record slab.
  void scatter_fp8_group(int group, const std::vector<int32_t>& ids,
                         const void* src, int group_size, uintptr_t stream,
                         bool checksum = false) {
    check_not_fp8_pages();
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    check_group_size(g, group_size);
    if (!gpu_mode_) {
      StorageOffloadEngine::host_fp8_group_copy(
          g, ids, const_cast<uint8_t*>(static_cast<const uint8_t*>(src)),
          group_size, /*quantize=*/false, footer(checksum), kv_dtype_);
      return;
    }
    hipError_t err = kvc_launch_scatter_fp8_group(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, group_size, ids.data(), static_cast<int>(ids.size()),
        nullptr, static_cast<const uint8_t*>(src),
        reinterpret_cast<hipStream_t>(stream), footer(checksum),
        static_cast<int>(kv_dtype_));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Group-scaled fp4 (e2m1) record size: n/2 code bytes + one f32 scale per
  // group_size elements, per tile; n = block_bytes/2 elements for 16-bit
  // pages, block_bytes for fp8 pages.
  size_t packed_bytes_fp4_group(int group, size_t n_blocks, int group_size,
                                bool checksum = false) const {
    const GroupDesc& g = groups_.at(group);
    check_fp4_group_size(g, group_size);
    return n_blocks * g.layer_ptrs.size() *
           (StorageOffloadEngine::fp4_group_record_bytes(
                g.block_bytes, group_size, kv_dtype_) +
            footer(checksum));
  }

  // Single-pass gather + per-group fp4 quantize into dst (device ptr in GPU
  // mode); needs no scratch. Host mode uses the software twin.
  void gather_fp4_group(int group, const std::vector<int32_t>& ids, void* dst,
                        int group_size, uintptr_t stream,
                        bool checksum = false) {
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    check_fp4_group_size(g, group_size);
    if (!gpu_mode_) {
      StorageOffloadEngine::host_fp4_group_copy(
          g, ids, static_cast<uint8_t*>(dst), group_size, /*quantize=*/true,
          footer(checksum), kv_dtype_);
      return;
    }
    hipError_t err = kvc_launch_gather_fp4_group(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, group_size, ids.data(), static_cast<int>(ids.size()),
        nullptr, static_cast<uint8_t*>(dst),
        reinterpret_cast<hipStream_t>(stream), footer(checksum),
        static_cast<int>(kv_dtype_));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Dequantize + scatter from a group-scaled fp4 record slab.
  void scatter_fp4_group(int group, const std::vector<int32_t>& ids,
                         const void* src, int group_size, uintptr_t stream,
                         bool checksum = false) {
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    check_fp4_group_size(g, group_size);
    if (!gpu_mode_) {
      StorageOffloadEngine::host_fp4_group_copy(
          g, ids, const_cast<uint8_t*>(static_cast<const uint8_t*>(src)),
          group_size, /*quantize=*/false, footer(checksum), kv_dtype_);
      return;
    }
    hipError_t err = kvc_launch_scatter_fp4_group(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, group_size, ids.data(), static_cast<int>(ids.size()),
        nullptr, static_cast<const uint8_t*>(src),
        reinterpret_cast<hipStream_t>(stream), footer(checksum),
        static_cast<int>(kv_dtype_));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  // Gather block_ids of `group` into contiguous dst (device ptr in GPU
  // mode). Async on `stream`; caller synchronizes.
  void gather(int group, const std::vector<int32_t>& ids, void* dst,
              uintptr_t stream, bool checksum = false) {
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    if (!gpu_mode_) {
      host_copy(g, ids, static_cast<uint8_t*>(dst), /*to_packed=*/true,
                footer(checksum));
      return;
    }
    hipError_t err = kvc_launch_gather(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, ids.data(), static_cast<int>(ids.size()), nullptr,
        static_cast<uint8_t*>(dst), reinterpret_cast<hipStream_t>(stream),
        footer(checksum));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

  void scatter(int group, const std::vector<int32_t>& ids, const void* src,
               uintptr_t stream, bool checksum = false) {
    const GroupDesc& g = groups_.at(group);
    check_ids(ids, g);
    if (!gpu_mode_) {
      host_copy(g, ids, const_cast<uint8_t*>(static_cast<const uint8_t*>(src)),
                /*to_packed=*/false, footer(checksum));
      return;
    }
    hipError_t err = kvc_launch_scatter(
        const_cast<const void* const*>(dev_layer_ptrs_[group]),
        dev_layer_strides_[group], static_cast<int>(g.layer_ptrs.size()),
        g.block_bytes, ids.data(), static_cast<int>(ids.size()), nullptr,
        static_cast<const uint8_t*>(src), reinterpret_cast<hipStream_t>(stream),
        footer(checksum));
    if (err != hipSuccess) throw HipError(hipGetErrorString(err));
  }

 private:
  static uint32_t footer(bool checksum) {
    return checksum ? static_cast<uint32_t>(kChecksumFooterBytes) : 0;
  }

  static void check_records(const void* slab, size_t tiles,
                            size_t payload_bytes) {
    if (slab == nullptr || tiles == 0 || tiles > 0xffffffffull)
      throw std::invalid_argument("need a slab of 1..2^32-1 records");
    if (payload_bytes == 0 || payload_bytes % 4 != 0 ||
        payload_bytes > 0xfffffff0ull)
      throw std::invalid_argument(
          "payload_bytes must be a positive multiple of 4 below 4 GiB");
    if (reinterpret_cast<uintptr_t>(slab) % 4 != 0)
      throw std::invalid_argument("record slab must be 4-byte aligned");
  }

  // csum_mu_ held. The scratch slab only grows; growing frees the old one,
  // which waits for the device, so no launch still reads it.
  void ensure_csum_buffers(size_t tiles) {
    const size_t need = kvc_checksum_scratch_bytes(tiles);
    if (need > csum_scratch_bytes_) {
      if (csum_scratch_) KVO_HIP_CHECK(hipFree(csum_scratch_));
      csum_scratch_ = nullptr;
      csum_scratch_bytes_ = 0;
      void* p = nullptr;
      KVO_HIP_CHECK(hipMalloc(&p, need));
      csum_scratch_ = static_cast<uint64_t*>(p);
      csum_scratch_bytes_ = need;
    }
    if (!csum_result_)
      csum_result_ = std::make_unique<HostStaging>(64, true, /*mapped=*/true);
  }

  static void check_ids(const std::vector<int32_t>& ids, const GroupDesc& g) {
    if (ids.empty() || ids.size() > kMaxBlocksPerFileHost)
      throw std::invalid_argument("block count must be in [1, 128]");
    if (g.num_blocks > 0) {
      for (int32_t id : ids)
        if (id < 0 || id >= g.num_blocks)
          throw std::invalid_argument("block id out of range");
    }
  }

  static void check_group_size(const GroupDesc& g, int group_size) {
    if (!fp8_group_size_ok(group_size))
      throw std::invalid_argument(
          "fp8 group_size must be 64, 128, 256 or 512 (got " +
          std::to_string(group_size) + ")");
    if (g.block_bytes % 16 != 0 || (g.block_bytes / 2) % group_size != 0)
      throw std::invalid_argument(
          "block_bytes/2 = " + std::to_string(g.block_bytes / 2) +
          " elements is not a multiple of fp8 group_size " +
          std::to_string(group_size));
  }

  void check_fp4_group_size(const GroupDesc& g, int group_size) const {
    if (!fp4_group_size_ok(group_size))
      throw std::invalid_argument(
          "fp4 group_size must be 16, 32, 64 or 128 (got " +
          std::to_string(group_size) + ")");
    const uint64_t n = kv_tile_elems(g.block_bytes, kv_dtype_);
    if (g.block_bytes % 16 != 0 || n % group_size != 0)
      throw std::invalid_argument(
          std::string(kv_dtype_ == KvDtype::kFp8E4M3 ? "block_bytes = "
                                                     : "block_bytes/2 = ") +
          std::to_string(n) + " elements is not a multiple of fp4 group_size " +
          std::to_string(group_size));
  }

  void check_not_fp8_pages() const {
    if (kv_dtype_ == KvDtype::kFp8E4M3)
      throw std::invalid_argument(
          "kv_dtype float8_e4m3fn: the pages already are fp8, the fp8 methods "
          "do not apply; use the raw or the fp4_group methods");
  }

  void host_copy(const GroupDesc& g, const std::vector<int32_t>& ids,
                 uint8_t* packed, bool to_packed, size_t footer) const {
    const size_t nl = g.layer_ptrs.size();
    const size_t rec = g.block_bytes + footer;
    for (size_t bi = 0; bi < ids.size(); ++bi) {
      for (size_t l = 0; l < nl; ++l) {
        uint8_t* page = static_cast<uint8_t*>(g.layer_ptrs[l]) +
                        static_cast<uint64_t>(ids[bi]) * g.layer_strides[l];
        uint8_t* slab = packed + (bi * nl + l) * rec;
        if (to_packed)
          std::memcpy(slab, page, g.block_bytes);
        else
          std::memcpy(page, slab, g.block_bytes);
      }
    }
  }

  void host_fp8(const GroupDesc& g, const std::vector<int32_t>& ids,
                uint8_t* packed, bool quantize, size_t footer) const {
    // software codec shared with the engine's host mode
    StorageOffloadEngine::host_fp8_copy(g, ids, packed, quantize, footer,
                                        kv_dtype_);
  }

  std::vector<GroupDesc> groups_;
  bool gpu_mode_;
  KvDtype kv_dtype_;
  std::vector<void**> dev_layer_ptrs_;
  std::vector<uint64_t*> dev_layer_strides_;
  std::mutex csum_mu_;
  uint64_t* csum_scratch_ = nullptr;
  size_t csum_scratch_bytes_ = 0;
  std::unique_ptr<HostStaging> csum_result_;
};

}  // namespace kvo
