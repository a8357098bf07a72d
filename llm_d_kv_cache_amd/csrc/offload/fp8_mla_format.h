// Geometry of serialize="fp8_ds_mla" records, shared by the kernels
// (kernels.hip) and their host twins (engine.h). Plain constants only, so
// both the device and the host compile can include it.
//
// An MLA page is a run of token rows of 576 16-bit elements: 512 compressed
// latent values (kv_lora_rank) followed by 64 RoPE key values. A row is
// stored as one 656-byte entry
//   [ 512 e4m3fn codes | 4 f32 scales, one per 128 latent values |
//     the 64 RoPE values, byte for byte ]
// and a tile record is its rows' entries back to back. 656 = 41 * 16 and
// 528 = 33 * 16, so every field of every entry is 16-byte aligned in a
// 16-byte aligned slab.
#pragma once

#include <cstdint>

namespace kvo {

constexpr uint32_t kMlaRowElems = 576;     // 16-bit elements per token row
constexpr uint32_t kMlaLatentElems = 512;  // quantized prefix of a row
constexpr uint32_t kMlaGroupElems = 128;   // latent elements per f32 scale
constexpr uint32_t kMlaRopeElems = kMlaRowElems - kMlaLatentElems;
constexpr uint32_t kMlaGroups = kMlaLatentElems / kMlaGroupElems;
constexpr uint32_t kMlaRowBytes = 2 * kMlaRowElems;                // 1152
constexpr uint32_t kMlaScaleOffset = kMlaLatentElems;              // 512
constexpr uint32_t kMlaRopeOffset = kMlaScaleOffset + 4 * kMlaGroups;  // 528
constexpr uint32_t kMlaEntryBytes = kMlaRopeOffset + 2 * kMlaRopeElems;  // 656

static_assert(kMlaRowBytes == 1152 && kMlaEntryBytes == 656, "fp8_ds_mla");
static_assert(kMlaRopeOffset % 16 == 0 && kMlaEntryBytes % 16 == 0,
              "entry fields are 16-byte aligned");

}  // namespace kvo
