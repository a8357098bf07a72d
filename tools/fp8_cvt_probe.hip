// What does v_cvt_pk_fp8_f32 return for -0.0 and for a negative that
// underflows, and does it agree with the host twin (engine.h f32_to_fp8_rne)
// on every product value(code) * scale the fp4-over-fp8-pages encoders can
// write? Also checks that v_cvt_f32_fp8 / v_cvt_pk_f32_fp8 widen every
// finite e4m3fn code exactly. Results: profiles/fp8_page_fp4_kernels.md.
//
//   hipcc --offload-arch=gfx950 -O2 -o fp8_cvt_probe tools/fp8_cvt_probe.hip
//   ./fp8_cvt_probe
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

__global__ void probe(const float* in, uint8_t* lo, uint8_t* hi, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t a = __builtin_amdgcn_cvt_pk_fp8_f32(in[i], 0.0f, 0u, false);
  uint32_t b = __builtin_amdgcn_cvt_pk_fp8_f32(0.0f, in[i], 0u, true);
  lo[i] = static_cast<uint8_t>(a);
  hi[i] = static_cast<uint8_t>(b >> 24);
}

__global__ void widen(float* out) {
  int i = threadIdx.x;  // 256 codes
  out[i] = __builtin_amdgcn_cvt_f32_fp8(static_cast<uint32_t>(i), 0);
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 p = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<uint32_t>(i) << 24, true);
  out[256 + i] = p.y;
}

static uint8_t f32_to_fp8_rne(float x) {
  uint32_t w;
  std::memcpy(&w, &x, 4);
  const uint32_t sign = (w >> 24) & 0x80u;
  w &= 0x7fffffffu;
  float a;
  std::memcpy(&a, &w, 4);
  const float f = a * 512.0f + 12582912.0f;
  uint32_t sub;
  std::memcpy(&sub, &f, 4);
  sub &= 0xffu;
  const uint32_t r = w + 0x7ffffu + ((w >> 20) & 1);
  uint32_t code = (r >> 20) - ((127u - 7u) << 3);
  code = code > 0x7eu ? 0x7eu : code;
  code = a < 0.015625f ? sub : code;
  return static_cast<uint8_t>(sign | code);
}

static float fp8_to_f32(uint8_t b) {
  int e = (b >> 3) & 0xf, m = b & 7;
  float v = e == 0 ? m * 0.001953125f : std::ldexp(1.0f + m / 8.0f, e - 7);
  return (b & 0x80) ? -v : v;
}

#define CK(x)                                                     \
  do {                                                            \
    hipError_t e_ = (x);                                          \
    if (e_ != hipSuccess) {                                       \
      std::printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); \
      return 2;                                                   \
    }                                                             \
  } while (0)

int main() {
  std::vector<float> in;
  const float named[] = {-0.0f, 0.0f, -std::ldexp(1.0f, -10), -std::ldexp(1.0f, -11),
                         -std::ldexp(1.0f, -20), -1e-30f, std::ldexp(1.0f, -10),
                         -std::ldexp(1.5f, -10), 448.0f, -448.0f, 448.00003f, 463.9f};
  const int n_named = sizeof(named) / sizeof(named[0]);
  for (float f : named) in.push_back(f);
  static const float kMag[8] = {0, 0.5f, 1, 1.5f, 2, 3, 4, 6};
  for (int a = 1; a < 0x7f; ++a) {
    const float scale = fp8_to_f32(static_cast<uint8_t>(a)) / 6.0f;
    for (int c = 0; c < 16; ++c) {
      float m = kMag[c & 7];
      in.push_back(((c & 8) ? -m : m) * scale);
    }
  }
  const int n = static_cast<int>(in.size());
  float* din;
  uint8_t *dlo, *dhi;
  float* dw;
  CK(hipMalloc(&din, n * 4));
  CK(hipMalloc(&dlo, n));
  CK(hipMalloc(&dhi, n));
  CK(hipMalloc(&dw, 512 * 4));
  CK(hipMemcpy(din, in.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, din, dlo, dhi, n);
  hipLaunchKernelGGL(widen, dim3(1), dim3(256), 0, 0, dw);
  CK(hipDeviceSynchronize());
  std::vector<uint8_t> lo(n), hi(n);
  std::vector<float> w(512);
  CK(hipMemcpy(lo.data(), dlo, n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(hi.data(), dhi, n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(w.data(), dw, 512 * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < n_named; ++i)
    std::printf("x=%-14.8g (bits %08x) -> lo 0x%02x hi 0x%02x  host 0x%02x\n", in[i],
                *reinterpret_cast<uint32_t*>(&in[i]), lo[i], hi[i],
                f32_to_fp8_rne(in[i]));
  int bad = 0, bad_sign_only = 0;
  for (int i = n_named; i < n; ++i) {
    uint8_t want = f32_to_fp8_rne(in[i]);
    if (lo[i] != want || hi[i] != want) {
      ++bad;
      if ((lo[i] & 0x7f) == (want & 0x7f) && (hi[i] & 0x7f) == (want & 0x7f))
        ++bad_sign_only;
      if (bad <= 10)
        std::printf("MISMATCH x=%.9g lo 0x%02x hi 0x%02x host 0x%02x\n", in[i],
                    lo[i], hi[i], want);
    }
  }
  std::printf("products: %d of %d differ from host RNE (%d in the sign bit only)\n",
              bad, n - n_named, bad_sign_only);
  int wbad = 0;
  for (int i = 0; i < 256; ++i) {
    if ((i & 0x7f) == 0x7f) continue;
    float want = fp8_to_f32(static_cast<uint8_t>(i));
    if (std::memcmp(&w[i], &want, 4) != 0 || std::memcmp(&w[256 + i], &want, 4) != 0) {
      ++wbad;
      if (wbad <= 5) std::printf("WIDEN code 0x%02x -> %g / %g want %g\n", i, w[i], w[256 + i], want);
    }
  }
  std::printf("widen: %d of 254 finite codes differ bitwise\n", wbad);
  return 0;
}
