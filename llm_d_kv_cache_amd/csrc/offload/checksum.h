// Per-record checksums: the host twin of kvc_seal_records /
// kvc_verify_records (kernels.hip).
//
// With EngineConfig::checksum a tile record is [ payload | footer ]:
//   footer bytes 0..7   sum            u64, little-endian
//          bytes 8..11  magic          0x5343564B ("KVCS")
//          bytes 12..15 payload_bytes  P as u32
// sum = SUM_i h(((i + 1) << 32) | w[i]) mod 2^64 over the payload's
// little-endian u32 words, h = the splitmix64 finalizer. The sum commutes,
// so the kernels may combine lane/wave/workgroup partials in any order and
// still land on the value computed here: host mode, the staged path and
// the zero-copy path write identical bytes.
//
// Records of the fp8 modes are only 4-byte aligned (stride n + 20), so
// every footer field moves through memcpy.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace kvo {

constexpr uint32_t kChecksumMagic = 0x5343564Bu;
constexpr size_t kChecksumFooterBytes = 16;

inline uint64_t checksum_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// payload_bytes % 4 == 0 (caller-checked).
inline uint64_t record_checksum(const uint8_t* payload, size_t payload_bytes) {
  uint64_t sum = 0;
  const size_t n = payload_bytes / 4;
  for (size_t i = 0; i < n; ++i) {
    uint32_t w;
    std::memcpy(&w, payload + 4 * i, 4);
    sum += checksum_mix((static_cast<uint64_t>(i + 1) << 32) | w);
  }
  return sum;
}

// Writes the footer of every record of a slab of `tiles` records with
// stride payload_bytes + 16, whatever the footers held before.
inline void seal_records_host(uint8_t* slab, size_t tiles,
                              size_t payload_bytes) {
  const size_t stride = payload_bytes + kChecksumFooterBytes;
  const uint32_t magic = kChecksumMagic;
  const uint32_t pb = static_cast<uint32_t>(payload_bytes);
  for (size_t t = 0; t < tiles; ++t) {
    uint8_t* rec = slab + t * stride;
    const uint64_t sum = record_checksum(rec, payload_bytes);
    std::memcpy(rec + payload_bytes, &sum, 8);
    std::memcpy(rec + payload_bytes + 8, &magic, 4);
    std::memcpy(rec + payload_bytes + 12, &pb, 4);
  }
}

// Returns the number of records whose footer does not match (all three
// fields must); *first_bad is the lowest such record index, -1 when none.
inline size_t verify_records_host(const uint8_t* slab, size_t tiles,
                                  size_t payload_bytes, int64_t* first_bad) {
  const size_t stride = payload_bytes + kChecksumFooterBytes;
  size_t bad = 0;
  *first_bad = -1;
  for (size_t t = 0; t < tiles; ++t) {
    const uint8_t* rec = slab + t * stride;
    uint64_t sum;
    uint32_t magic, pb;
    std::memcpy(&sum, rec + payload_bytes, 8);
    std::memcpy(&magic, rec + payload_bytes + 8, 4);
    std::memcpy(&pb, rec + payload_bytes + 12, 4);
    if (magic == kChecksumMagic && pb == static_cast<uint32_t>(payload_bytes) &&
        sum == record_checksum(rec, payload_bytes))
      continue;
    if (bad++ == 0) *first_bad = static_cast<int64_t>(t);
  }
  return bad;
}

}  // namespace kvo
