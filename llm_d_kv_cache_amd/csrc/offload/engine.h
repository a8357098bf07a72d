// StorageOffloadEngine: the KV-block offload job orchestrator.
//
// Capability parity with the reference StorageOffloadEngine
// (csrc/storage/storage_offload.cpp): async store/load of GPU KV blocks to
// content-addressed files, KV-ready event fencing against the serving
// engine's stream, per-file tasks on the NUMA-pinned I/O pool (loads HIGH
// priority), skip-if-exists dedupe with atime touch, EMA-driven dynamic
// write-queue limit with write dropping, job cancellation (preemption), and
// get_finished() polling.
//
// MI355X-first redesign of the copy path: the default "staged" mode runs
// the CDNA4 gather kernel HBM->HBM into a contiguous device bounce (brief,
// bandwidth-bound CU usage) and crosses PCIe with hipMemcpyAsync on the
// SDMA engines — zero CU occupancy while the wire is busy, so serving
// compute is undisturbed. "zero_copy" mode instead has the kernel write
// device-mapped pinned host memory directly (the reference's only mode).
// Constructed against host tensors the same control logic runs on memcpy
// ("host" mode, CPU-only CI) — an explicit mode, never a silent fallback.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <chrono>
#include <functional>
#include <thread>
#include <list>
#include <map>
#include <unordered_map>

#include "checksum.h"
#include "common.h"
#include "file_io.h"
#include "host_cache.h"
#include "pcie_mover.h"
#include "thread_pool.h"

// Launchers take host block ids (by-value kernarg, <=128) OR a device
// pointer (ids_dev != nullptr) for bigger transfers — no kernel-side
// blocks-per-file ceiling. The trailing uint32_t is the footer bytes every
// record carries behind its payload: 0 (dense layout) or 16 (checksums).
// The fp8 launchers end with the page format, a KvDtype as int; any other
// value returns hipErrorInvalidValue.
extern "C" hipError_t kvc_launch_gather(const void* const*, const uint64_t*, int,
                                        uint64_t, const int32_t*, int,
                                        const int32_t*, uint8_t*, hipStream_t,
                                        uint32_t);
extern "C" hipError_t kvc_launch_scatter(const void* const*, const uint64_t*, int,
                                         uint64_t, const int32_t*, int,
                                         const int32_t*, const uint8_t*,
                                         hipStream_t, uint32_t);
extern "C" hipError_t kvc_launch_gather_fp8(const void* const*, const uint64_t*,
                                            int, uint64_t, const int32_t*, int,
                                            const int32_t*, uint8_t*,
                                            hipStream_t, uint32_t, int);
extern "C" hipError_t kvc_launch_gather_fp8_split(
    const void* const*, const uint64_t*, int, uint64_t, const int32_t*, int,
    const int32_t*, uint8_t*, float*, hipStream_t, uint32_t, int);
extern "C" hipError_t kvc_launch_scatter_fp8(const void* const*, const uint64_t*,
                                             int, uint64_t, const int32_t*, int,
                                             const int32_t*, const uint8_t*,
                                             hipStream_t, uint32_t, int);
// group-scaled fp8: the int after block_bytes is the group size in elements
extern "C" hipError_t kvc_launch_gather_fp8_group(
    const void* const*, const uint64_t*, int, uint64_t, int, const int32_t*,
    int, const int32_t*, uint8_t*, hipStream_t, uint32_t, int);
extern "C" hipError_t kvc_launch_scatter_fp8_group(
    const void* const*, const uint64_t*, int, uint64_t, int, const int32_t*,
    int, const int32_t*, const uint8_t*, hipStream_t, uint32_t, int);
// group-scaled fp4 (e2m1): same argument lists as the fp8-group pair; the
// only launchers that also take KvDtype::kFp8E4M3 pages (block_bytes elements
// per tile instead of block_bytes/2)
extern "C" hipError_t kvc_launch_gather_fp4_group(
    const void* const*, const uint64_t*, int, uint64_t, int, const int32_t*,
    int, const int32_t*, uint8_t*, hipStream_t, uint32_t, int);
extern "C" hipError_t kvc_launch_scatter_fp4_group(
    const void* const*, const uint64_t*, int, uint64_t, int, const int32_t*,
    int, const int32_t*, const uint8_t*, hipStream_t, uint32_t, int);
// Record checksums (checksum.h has the format and the host twin). slab holds
// `tiles` records of payload_bytes + 16; scratch is
// kvc_checksum_scratch_bytes(tiles) of 8-byte aligned device memory; result
// is two device-writable u32 (bad count, first bad index).
extern "C" size_t kvc_checksum_scratch_bytes(size_t tiles);
extern "C" hipError_t kvc_launch_seal_records(uint8_t*, uint32_t, uint64_t,
                                              uint64_t*, hipStream_t);
extern "C" hipError_t kvc_launch_verify_records(const uint8_t*, uint32_t,
                                                uint64_t, uint64_t*, uint32_t*,
                                                hipStream_t);

namespace kvo {

constexpr int kMaxBlocksPerFileHost = 128;  // mirrors kernels.hip kMaxBlocksPerFile
constexpr int kMaxBlocksPerFileDev = 4096;  // via per-worker device id buffer

// Intra-transfer pipeline granularity: the PCIe hop and the file I/O of one
// transfer overlap at this chunk size (copy chunk i+1 rides the SDMA stream
// while chunk i is written/was read). Transfers at or below 64 MiB run
// single-shot: with 16 workers the pipeline across tasks already overlaps
// file I/O with the wire, and measured intra-task chunking at 32 MiB files
// only added memory-traffic contention (read-side accumulated time 3x).
constexpr size_t kPipelineChunkBytes = 16ull << 20;

inline size_t pipeline_chunk(size_t bytes) {
  return bytes <= 4 * kPipelineChunkBytes ? bytes : kPipelineChunkBytes;
}

enum class CopyPath { kStaged, kZeroCopy, kHostMemcpy };

// Payload serialization: raw bytes, or fp8 e4m3fn quantization of 16-bit
// float pages (halves wire + storage bytes; one f32 scale per (block, layer)
// tile appended to each tile record). kFp8E4M3Group scales every
// fp8_group_size-element run on its own (users set it to head_dim): the
// record is [ n fp8 | n/G f32 scales ], n = block_bytes/2. kFp4E2M1Group is
// the same design one step narrower: OCP e2m1 codes, two per byte, one f32
// scale per fp4_group_size elements; the record is
// [ n/2 code bytes | n/G f32 scales ].
enum class Serialize { kRaw, kFp8E4M3, kFp8E4M3Group, kFp4E2M1Group };

// Format of the KV pages the fp8 and fp4 modes read on store and write on
// load (raw copies never look at it). The records are format-free; only the
// page <-> f32 conversions differ. The values are the kv_dtype argument of
// the fp8 and fp4 launchers in kernels.hip. kFp8E4M3 pages (OCP e4m3fn, one
// byte per element) are a source of kFp4E2M1Group only: the fp8 modes have
// nothing to narrow and their launchers reject the value.
enum class KvDtype : int { kBf16 = 0, kFp16 = 1, kFp8E4M3 = 2 };

inline KvDtype parse_kv_dtype(const std::string& s) {
  if (s == "bfloat16") return KvDtype::kBf16;
  if (s == "float16") return KvDtype::kFp16;
  if (s == "float8_e4m3fn") return KvDtype::kFp8E4M3;
  throw std::invalid_argument(
      "kv_dtype must be bfloat16|float16|float8_e4m3fn (got '" + s + "')");
}

// Elements in a tile of block_bytes: two bytes each for bf16/fp16 pages, one
// for fp8 pages.
inline uint64_t kv_tile_elems(uint64_t block_bytes, KvDtype kv_dtype) {
  return kv_dtype == KvDtype::kFp8E4M3 ? block_bytes : block_bytes / 2;
}

inline bool fp8_group_size_ok(int g) {
  return g == 64 || g == 128 || g == 256 || g == 512;
}

inline bool fp4_group_size_ok(int g) {
  return g == 16 || g == 32 || g == 64 || g == 128;
}

// Store completion semantics: kThrough = the file rename happened (crash
// durable); kBack = the slab is resident in the pinned-DRAM tier and the
// file flush runs asynchronously (store latency ~= gather + D2H; loses
// only not-yet-flushed cache entries on crash — acceptable for a cache).
// kBack needs host_cache_bytes > 0; transfers that cannot get a slot fall
// back to write-through.
enum class WritePolicy { kThrough, kBack };

struct GroupDesc {
  std::vector<void*> layer_ptrs;        // per-layer block-0 base address
  std::vector<uint64_t> layer_strides;  // bytes between consecutive blocks
  uint64_t block_bytes = 0;             // bytes per (block, layer)
  int64_t num_blocks = 0;               // device pages per layer (0 = unchecked)
};

struct EngineConfig {
  int io_threads = 16;
  int gpu_blocks_per_file = 16;
  double read_preferring_ratio = 0.75;
  double max_write_queued_seconds = 30.0;
  bool gpu_mode = false;
  int device = 0;
  CopyPath copy_path = CopyPath::kStaged;
  Serialize serialize = Serialize::kRaw;
  int fp8_group_size = 128;  // elements per scale; kFp8E4M3Group only
  int fp4_group_size = 32;   // elements per scale; kFp4E2M1Group only
  // Pinned host-DRAM cache tier (0 = disabled): write-through on store,
  // cache-hit loads skip the filesystem (host_cache.h).
  size_t host_cache_bytes = 0;
  WritePolicy write_policy = WritePolicy::kThrough;
  // O_DIRECT file I/O (page-cache bypass for local NVMe; auto-fallback on
  // unsupported filesystems/unaligned transfers) — the GDS-substitute
  // mode (no cuFile exists on ROCm; see docs/architecture.md).
  bool direct_io = false;
  // Per-record checksums: every tile record gains a 16-byte footer
  // (checksum.h) that is sealed on store and verified on load before any KV
  // page is written. Files with and without footers must not share a
  // directory: tag the FileMapper dtype with "+ck" (docs/configuration.md).
  bool checksum = false;
  // Page format of the KV tensors; consulted only by the fp8 and fp4 modes.
  KvDtype kv_dtype = KvDtype::kBf16;
};

struct FileTransfer {
  int group = 0;
  std::string path;
  std::vector<int32_t> block_ids;
  // Block-slot offset of this span within the file's nominal layout. Stores
  // emit slot_offset == 0 (head-partial files are simply short); loads may
  // skip an already-cached head.
  int slot_offset = 0;
};

struct FinishedJob {
  int64_t id = 0;
  bool success = false;
  bool dropped = false;
};

struct EngineStats {
  uint64_t stores_submitted = 0;
  uint64_t loads_submitted = 0;
  uint64_t files_written = 0;
  uint64_t files_deduped = 0;
  uint64_t files_read = 0;
  uint64_t writes_dropped = 0;
  uint64_t tasks_cancelled = 0;
  uint64_t host_cache_hits = 0;
  uint64_t host_cache_stores = 0;
  uint64_t writeback_flushes = 0;
  uint64_t errors = 0;
  uint64_t checksum_failures = 0;  // records that failed verification
  double avg_write_seconds = 0;
  uint64_t bytes_stored = 0;
  uint64_t bytes_loaded = 0;
  // accumulated per-phase wall time across all workers (ms)
  double t_gather_ms = 0, t_d2h_ms = 0, t_write_ms = 0;
  double t_read_ms = 0, t_h2d_ms = 0, t_scatter_ms = 0;
  // PCIe lane utilization (mover-side truth: busy wall per direction)
  double d2h_lane_busy_ms = 0, h2d_lane_busy_ms = 0;
  uint64_t d2h_lane_bytes = 0, h2d_lane_bytes = 0;
};

class StorageOffloadEngine {
 public:
  StorageOffloadEngine(EngineConfig cfg, std::vector<GroupDesc> groups)
      : cfg_(cfg), groups_(std::move(groups)) {
    if (cfg_.gpu_blocks_per_file > kMaxBlocksPerFileDev)
      throw std::invalid_argument(
          "gpu_blocks_per_file exceeds engine limit (4096)");
    if (cfg_.gpu_mode) {
      // Transient init failures have been observed right after another
      // process released the device: retry briefly before giving up.
      int count = 0;
      hipError_t err = hipSuccess;
      for (int attempt = 0; attempt < 10; ++attempt) {
        err = hipGetDeviceCount(&count);
        if (err == hipSuccess && count > cfg_.device) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(200));
      }
      if (err != hipSuccess || count <= cfg_.device)
        throw HipError(std::string("gpu_mode requested but device ") +
                       std::to_string(cfg_.device) + " unavailable: " +
                       hipGetErrorString(err) + " (count=" +
                       std::to_string(count) + ")");
      KVO_HIP_CHECK(hipSetDevice(cfg_.device));
    } else {
      cfg_.copy_path = CopyPath::kHostMemcpy;
    }

    const bool grouped = cfg_.serialize == Serialize::kFp8E4M3Group;
    if (grouped && !fp8_group_size_ok(cfg_.fp8_group_size))
      throw std::invalid_argument(
          "fp8_group_size must be 64, 128, 256 or 512 (got " +
          std::to_string(cfg_.fp8_group_size) + ")");
    if (cfg_.kv_dtype == KvDtype::kFp8E4M3 &&
        (grouped || cfg_.serialize == Serialize::kFp8E4M3))
      throw std::invalid_argument(
          "kv_dtype float8_e4m3fn: the pages already are fp8, so the fp8 "
          "serialize modes do not apply; use raw or fp4_e2m1_group");
    const bool fp4 = cfg_.serialize == Serialize::kFp4E2M1Group;
    if (fp4 && !fp4_group_size_ok(cfg_.fp4_group_size))
      throw std::invalid_argument(
          "fp4_group_size must be 16, 32, 64 or 128 (got " +
          std::to_string(cfg_.fp4_group_size) + ")");
    // Staging is sized from raw block_bytes (the fp8 layouts are smaller and
    // the split fp8 gather keeps its scratch in the difference). With
    // footers raw is block_bytes + 16 per tile and nothing is left over, so
    // that mode sizes every buffer from the real record stride and gives
    // the device bounce its scratch tail explicitly.
    size_t max_file_bytes = 0;
    size_t max_device_bytes = 0;
    for (size_t gi = 0; gi < groups_.size(); ++gi) {
      auto& g = groups_[gi];
      if (g.block_bytes % 16 != 0)
        throw std::invalid_argument("block_bytes must be a multiple of 16");
      if (grouped && (g.block_bytes / 2) % cfg_.fp8_group_size != 0)
        throw std::invalid_argument(
            "group " + std::to_string(gi) + ": block_bytes/2 = " +
            std::to_string(g.block_bytes / 2) +
            " elements is not a multiple of fp8_group_size " +
            std::to_string(cfg_.fp8_group_size));
      if (fp4 &&
          kv_tile_elems(g.block_bytes, cfg_.kv_dtype) % cfg_.fp4_group_size != 0)
        throw std::invalid_argument(
            "group " + std::to_string(gi) + ": " +
            (cfg_.kv_dtype == KvDtype::kFp8E4M3 ? "block_bytes = "
                                                : "block_bytes/2 = ") +
            std::to_string(kv_tile_elems(g.block_bytes, cfg_.kv_dtype)) +
            " elements is not a multiple of fp4_group_size " +
            std::to_string(cfg_.fp4_group_size));
      if (g.layer_ptrs.size() != g.layer_strides.size())
        throw std::invalid_argument("layer ptr/stride length mismatch");
      if (cfg_.checksum) {
        const size_t tiles =
            static_cast<size_t>(cfg_.gpu_blocks_per_file) * g.layer_ptrs.size();
        const size_t fb = tiles * tile_record_bytes(g);
        max_file_bytes = std::max(max_file_bytes, fb);
        max_device_bytes =
            std::max(max_device_bytes, align16(fb) + scratch_bytes(tiles));
      } else {
        max_file_bytes = std::max(
            max_file_bytes, static_cast<size_t>(cfg_.gpu_blocks_per_file) *
                                g.layer_ptrs.size() * g.block_bytes);
        max_device_bytes = max_file_bytes;
      }
      if (cfg_.gpu_mode) {
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

    size_t device_staging =
        cfg_.copy_path == CopyPath::kStaged ? max_device_bytes : 0;
    bool mapped = cfg_.copy_path == CopyPath::kZeroCopy;
    pool_ = std::make_unique<IoThreadPool>(
        cfg_.io_threads, cfg_.gpu_mode, cfg_.device, max_file_bytes, device_staging,
        cfg_.read_preferring_ratio, mapped,
        /*verify_result=*/cfg_.checksum && cfg_.copy_path == CopyPath::kStaged);
    if (cfg_.gpu_mode && cfg_.copy_path == CopyPath::kStaged)
      mover_ = std::make_unique<PcieMover>(true, cfg_.device);
    if (cfg_.host_cache_bytes > 0 && cfg_.copy_path != CopyPath::kZeroCopy &&
        max_file_bytes > 0)
      cache_ = std::make_unique<HostPinnedCache>(cfg_.host_cache_bytes,
                                                 max_file_bytes, cfg_.gpu_mode);
  }

  ~StorageOffloadEngine() {
    pool_.reset();  // drain workers before freeing device arrays
    for (auto p : dev_layer_ptrs_) (void)hipFree(p);
    for (auto p : dev_layer_strides_) (void)hipFree(p);
  }

  const EngineConfig& config() const { return cfg_; }

  // Peer/DRAM-tier bridge: copy a resident host-cache entry for `path` into
  // caller memory so a peer GPU can be served over xGMI even after the
  // blocks left HBM. Returns payload bytes on hit, -1 on miss, -2 when cap
  // is too small. The copy (vs handing out the slot) decouples the pinned
  // slab's lifetime from the caller's async send.
  int64_t host_cache_read(const std::string& path, uint8_t* dst, size_t cap) {
    if (!cache_) return -1;
    HostPinnedCache::Slot* s = cache_->lookup(path);
    if (s == nullptr) return -1;
    const size_t n = s->bytes_used;
    if (n > cap) {
      cache_->release(s);
      return -2;
    }
    std::memcpy(dst, s->buf->host(), n);
    cache_->release(s);
    return static_cast<int64_t>(n);
  }

  // ---- store ----------------------------------------------------------------

  int64_t async_store(std::vector<FileTransfer> files, uintptr_t caller_stream) {
    // Validate EVERYTHING before any task is enqueued: a throw mid-list
    // after partial enqueue would leave job->remaining never reaching 0
    // (wait_job deadlock, pending_writes_ leak).
    for (const auto& ft : files) validate(ft);
    auto job = new_job(files.size(), /*is_store=*/true);
    if (files.empty()) {
      complete_empty(job);
      return job->id;
    }

    // Dynamic write-queue limit (EMA of write duration): when the backlog
    // exceeds threads * max_queued_seconds / avg_write_seconds, the whole
    // store is dropped — offload is a cache, dropping is always safe.
    {
      double avg = avg_write_seconds();
      if (avg > 0) {
        size_t limit = static_cast<size_t>(
            pool_->size() * cfg_.max_write_queued_seconds / avg);
        if (pending_writes_.load(std::memory_order_relaxed) > limit) {
          stats_inc([&](EngineStats& s) { s.writes_dropped += files.size(); });
          std::lock_guard<std::mutex> g(jobs_mu_);
          job->remaining = 0;
          finished_.push_back({job->id, true, /*dropped=*/true});
          jobs_.erase(job->id);
          done_cv_.notify_all();
          return job->id;
        }
      }
      pending_writes_.fetch_add(files.size(), std::memory_order_relaxed);
    }

    if (cfg_.gpu_mode) {
      KVO_HIP_CHECK(hipEventCreateWithFlags(&job->kv_ready, hipEventDisableTiming));
      KVO_HIP_CHECK(hipEventRecord(job->kv_ready,
                                   reinterpret_cast<hipStream_t>(caller_stream)));
    }
    stats_inc([&](EngineStats& s) { s.stores_submitted += files.size(); });

    for (auto& ft : files) {
      pool_->enqueue(Priority::kNormal, [this, job, ft](WorkerCtx& ctx) {
        bool ok = true;
        double t0 = now_s();
        bool wrote = false;
        bool deferred = false;
        try {
          if (!job->cancelled.load(std::memory_order_acquire)) {
            if (file_exists(ft.path)) {
              touch_atime(ft.path);
              stats_inc([](EngineStats& s) { s.files_deduped++; });
            } else {
              deferred = store_one(ctx, job, ft);
              wrote = !deferred;
            }
          } else {
            stats_inc([](EngineStats& s) { s.tasks_cancelled++; });
          }
        } catch (const std::exception& e) {
          KVO_LOG_ERROR("store %s failed: %s", ft.path.c_str(), e.what());
          stats_inc([](EngineStats& s) { s.errors++; });
          ok = false;
        }
        if (deferred) return;  // write continuation owns EMA/pending/done
        if (wrote) update_write_ema(now_s() - t0);
        pending_writes_.fetch_sub(1, std::memory_order_relaxed);
        task_done(job, ok);
      });
    }
    return job->id;
  }

  // ---- load -----------------------------------------------------------------

  int64_t async_load(std::vector<FileTransfer> files) {
    for (const auto& ft : files) validate(ft);  // before ANY enqueue (see store)
    auto job = new_job(files.size(), /*is_store=*/false);
    if (files.empty()) {
      complete_empty(job);
      return job->id;
    }
    stats_inc([&](EngineStats& s) { s.loads_submitted += files.size(); });
    for (auto& ft : files) {
      pool_->enqueue(Priority::kHigh, [this, job, ft](WorkerCtx& ctx) {
        bool ok = true;
        try {
          if (!job->cancelled.load(std::memory_order_acquire)) {
            load_one(ctx, ft);
          } else {
            stats_inc([](EngineStats& s) { s.tasks_cancelled++; });
          }
        } catch (const std::exception& e) {
          KVO_LOG_ERROR("load %s failed: %s", ft.path.c_str(), e.what());
          stats_inc([](EngineStats& s) { s.errors++; });
          ok = false;
        }
        task_done(job, ok);
      });
    }
    return job->id;
  }

  // ---- completion -----------------------------------------------------------

  std::vector<FinishedJob> get_finished() {
    std::lock_guard<std::mutex> g(jobs_mu_);
    std::vector<FinishedJob> out;
    out.swap(finished_);
    return out;
  }

  // Non-blocking cancel: queued tasks of the job bail when dequeued.
  // Returns false when the job already finished. Preemption sets flags for
  // every affected job FIRST, then waits — a combined cancel+wait per job
  // always loses the race against the worker's next dequeue.
  bool cancel_job(int64_t id) {
    std::lock_guard<std::mutex> g(jobs_mu_);
    auto it = jobs_.find(id);
    if (it == jobs_.end()) return false;
    it->second->cancelled.store(true, std::memory_order_release);
    return true;
  }

  // Cancel a job's queued tasks (preemption) and wait for in-flight ones.
  // Returns true when every task that DID run succeeded.
  bool wait_job(int64_t id) {
    std::shared_ptr<Job> job;
    {
      std::lock_guard<std::mutex> g(jobs_mu_);
      auto it = jobs_.find(id);
      if (it == jobs_.end()) return true;  // already finished
      job = it->second;
    }
    job->cancelled.store(true, std::memory_order_release);
    std::unique_lock<std::mutex> g(jobs_mu_);
    done_cv_.wait(g, [&] { return job->remaining.load() == 0; });
    return job->success.load();
  }

  EngineStats stats() {
    EngineStats out;
    for (auto& sh : stats_shards_) {
      std::lock_guard<std::mutex> g(sh.mu);
      const EngineStats& s = sh.s;
      out.stores_submitted += s.stores_submitted;
      out.loads_submitted += s.loads_submitted;
      out.files_written += s.files_written;
      out.files_deduped += s.files_deduped;
      out.files_read += s.files_read;
      out.writes_dropped += s.writes_dropped;
      out.tasks_cancelled += s.tasks_cancelled;
      out.host_cache_hits += s.host_cache_hits;
      out.host_cache_stores += s.host_cache_stores;
      out.writeback_flushes += s.writeback_flushes;
      out.errors += s.errors;
      out.checksum_failures += s.checksum_failures;
      out.bytes_stored += s.bytes_stored;
      out.bytes_loaded += s.bytes_loaded;
      out.t_gather_ms += s.t_gather_ms;
      out.t_d2h_ms += s.t_d2h_ms;
      out.t_write_ms += s.t_write_ms;
      out.t_read_ms += s.t_read_ms;
      out.t_h2d_ms += s.t_h2d_ms;
      out.t_scatter_ms += s.t_scatter_ms;
    }
    out.avg_write_seconds = avg_write_seconds();
    if (mover_) {
      auto d = mover_->lane_stats(0), h = mover_->lane_stats(1);
      out.d2h_lane_busy_ms = d.busy_s * 1e3;
      out.h2d_lane_busy_ms = h.busy_s * 1e3;
      out.d2h_lane_bytes = d.bytes;
      out.h2d_lane_bytes = h.bytes;
    }
    return out;
  }

  size_t pending_writes() {
    return pending_writes_.load(std::memory_order_relaxed);
  }

 private:
  struct Job {
    int64_t id;
    std::atomic<int> remaining{0};
    std::atomic<bool> cancelled{false};
    std::atomic<bool> success{true};
    hipEvent_t kv_ready = nullptr;
  };

  void validate(const FileTransfer& ft) {
    if (ft.group < 0 || ft.group >= static_cast<int>(groups_.size()))
      throw std::invalid_argument("bad group index");
    if (ft.block_ids.empty() ||
        ft.block_ids.size() > static_cast<size_t>(cfg_.gpu_blocks_per_file))
      throw std::invalid_argument("bad block count for file transfer");
    int64_t nb = groups_[ft.group].num_blocks;
    if (nb > 0) {
      for (int32_t id : ft.block_ids)
        if (id < 0 || id >= nb)
          throw std::invalid_argument(
              "block id " + std::to_string(id) + " out of range [0, " +
              std::to_string(nb) + ")");
    }
  }

  void complete_empty(const std::shared_ptr<Job>& job) {
    std::lock_guard<std::mutex> g(jobs_mu_);
    finished_.push_back({job->id, true, false});
    jobs_.erase(job->id);
    done_cv_.notify_all();
  }

  std::shared_ptr<Job> new_job(size_t n_tasks, bool) {
    auto job = std::make_shared<Job>();
    std::lock_guard<std::mutex> g(jobs_mu_);
    job->id = next_job_id_++;
    job->remaining = static_cast<int>(n_tasks);
    jobs_[job->id] = job;
    return job;
  }

  void task_done(const std::shared_ptr<Job>& job, bool ok) {
    if (!ok) job->success.store(false, std::memory_order_relaxed);
    if (job->remaining.fetch_sub(1, std::memory_order_acq_rel) == 1) {
      if (job->kv_ready) {
        (void)hipEventDestroy(job->kv_ready);
        job->kv_ready = nullptr;
      }
      std::lock_guard<std::mutex> g(jobs_mu_);
      finished_.push_back({job->id, job->success.load(), false});
      jobs_.erase(job->id);
      done_cv_.notify_all();
    }
  }

  // Per-thread-sharded stats: phase-timing updates run ~6x per task from
  // every worker, so they must not contend on the job-completion mutex
  // (or each other). Each worker thread maps to one shard; stats()
  // aggregates.
  static constexpr size_t kStatsShards = 32;
  struct alignas(64) StatsShard {
    std::mutex mu;
    EngineStats s;
  };

  template <typename F>
  void stats_inc(F f) {
    thread_local size_t idx =
        std::hash<std::thread::id>{}(std::this_thread::get_id()) % kStatsShards;
    auto& sh = stats_shards_[idx];
    std::lock_guard<std::mutex> g(sh.mu);
    f(sh.s);
  }

  double avg_write_seconds() const {
    uint64_t bits = write_ema_bits_.load(std::memory_order_relaxed);
    double v;
    std::memcpy(&v, &bits, 8);
    return v;
  }

  void update_write_ema(double dt) {
    // EMA alpha=0.05 of write duration drives the queue limit; lock-free
    // CAS keeps it off the completion mutex.
    uint64_t old_bits = write_ema_bits_.load(std::memory_order_relaxed);
    for (;;) {
      double old_v;
      std::memcpy(&old_v, &old_bits, 8);
      double new_v = old_v == 0 ? dt : 0.95 * old_v + 0.05 * dt;
      uint64_t new_bits;
      std::memcpy(&new_bits, &new_v, 8);
      if (write_ema_bits_.compare_exchange_weak(old_bits, new_bits,
                                                std::memory_order_relaxed))
        return;
    }
  }

  // Bytes of a tile record before the optional checksum footer.
  size_t tile_payload_bytes(const GroupDesc& g) const {
    switch (cfg_.serialize) {
      case Serialize::kFp8E4M3:
        return g.block_bytes / 2 + 4;
      case Serialize::kFp8E4M3Group:
        return fp8_group_record_bytes(g.block_bytes, cfg_.fp8_group_size);
      case Serialize::kFp4E2M1Group:
        return fp4_group_record_bytes(g.block_bytes, cfg_.fp4_group_size,
                                      cfg_.kv_dtype);
      default:
        return g.block_bytes;
    }
  }

  uint32_t footer_bytes() const {
    return cfg_.checksum ? static_cast<uint32_t>(kChecksumFooterBytes) : 0;
  }

  size_t tile_record_bytes(const GroupDesc& g) const {
    return tile_payload_bytes(g) + footer_bytes();
  }

  static size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

  // Device scratch behind a checksummed slab of `tiles` records: the
  // partial sums of seal/verify, which also covers the partial maxima of
  // the split fp8 gather (4 bytes each where these take 8, and consumed
  // on the same stream before seal starts).
  static size_t scratch_bytes(size_t tiles) {
    return kvc_checksum_scratch_bytes(tiles);
  }

  uint64_t* checksum_scratch(WorkerCtx& ctx, size_t bytes) const {
    return reinterpret_cast<uint64_t*>(ctx.device_staging->ptr() +
                                       align16(bytes));
  }

  struct ChecksumError : std::runtime_error {
    using std::runtime_error::runtime_error;
  };

  // A span failed verification: count it, remove every copy that could
  // fail again (the store path skips files that exist, so a poisoned file
  // would otherwise fail forever), and fail the task. The caller has not
  // written a KV page yet; an in-flight fill slot is abandoned by its guard.
  [[noreturn]] void checksum_failed(const FileTransfer& ft, size_t nl,
                                    size_t bad, int64_t first,
                                    const char* source) {
    stats_inc([&](EngineStats& s) { s.checksum_failures += bad; });
    if (cache_) cache_->invalidate(ft.path);
    ::unlink(ft.path.c_str());
    const int64_t tile = static_cast<int64_t>(ft.slot_offset) *
                             static_cast<int64_t>(nl) + first;
    throw ChecksumError("checksum mismatch in " + std::string(source) + " " +
                        ft.path + ": " + std::to_string(bad) +
                        " bad record(s), first bad tile " +
                        std::to_string(tile) + " (block slot " +
                        std::to_string(tile / static_cast<int64_t>(nl)) +
                        ", layer " +
                        std::to_string(tile % static_cast<int64_t>(nl)) +
                        "); copy removed");
  }

  void verify_host(const FileTransfer& ft, const GroupDesc& g, size_t tiles,
                   const uint8_t* slab, const char* source) {
    int64_t first = -1;
    const size_t bad =
        verify_records_host(slab, tiles, tile_payload_bytes(g), &first);
    if (bad != 0)
      checksum_failed(ft, g.layer_ptrs.size(), bad, first, source);
  }

  size_t file_bytes(const GroupDesc& g, size_t n_blocks) const {
    return n_blocks * g.layer_ptrs.size() * tile_record_bytes(g);
  }

  // Two-stage store A/B switch (KVC_TWO_STAGE=1 opts in). Measured SLOWER
  // than the serial per-worker D2H->write flow on every box tried (same-
  // box: 52.0 vs 55.4 GB/s at 32 workers, 42.9 vs 49.1 at 16): splitting
  // the write off starves the D2H queue worse than the write blocking the
  // worker does, because submission — not lane service — is the scarce
  // resource. Kept for future re-measurement; default off.
  static bool two_stage_stores() {
    static const bool on = [] {
      const char* e = std::getenv("KVC_TWO_STAGE");
      return e != nullptr && e[0] == '1';
    }();
    return on;
  }

  // Block ids above the kernarg limit ride the worker's device buffer.
  const int32_t* stage_ids(WorkerCtx& ctx, const FileTransfer& ft) {
    if (ft.block_ids.size() <= static_cast<size_t>(kMaxBlocksPerFileHost))
      return nullptr;
    KVO_HIP_CHECK(hipMemcpyAsync(ctx.dev_ids, ft.block_ids.data(),
                                 ft.block_ids.size() * sizeof(int32_t),
                                 hipMemcpyHostToDevice, ctx.stream));
    return ctx.dev_ids;
  }

  // Returns true when completion was DEFERRED to a write-continuation task
  // (two-stage store): the caller must then skip EMA/pending/task_done.
  bool store_one(WorkerCtx& ctx, const std::shared_ptr<Job>& job,
                 const FileTransfer& ft) {
    const GroupDesc& g = groups_[ft.group];
    const int nb = static_cast<int>(ft.block_ids.size());
    const int nl = static_cast<int>(g.layer_ptrs.size());
    const size_t bytes = file_bytes(g, nb);

    HostPinnedCache::Slot* slot =
        cache_ ? cache_->acquire(ft.path, bytes) : nullptr;
    uint8_t* host_buf = slot ? slot->buf->host() : ctx.host_staging->host();
    struct SlotGuard {
      HostPinnedCache* c;
      HostPinnedCache::Slot* s;
      bool ok = false;
      ~SlotGuard() {
        if (!c || !s) return;
        if (ok) {
          c->publish(s);
          c->release(s);
        } else {
          c->abandon(s);
        }
      }
    } guard{cache_.get(), slot};

    if (cfg_.copy_path == CopyPath::kHostMemcpy) {
      gather_host(g, ft.block_ids, host_buf);
      if (cfg_.checksum)
        seal_records_host(host_buf, static_cast<size_t>(nb) * nl,
                          tile_payload_bytes(g));
      if (cfg_.write_policy == WritePolicy::kBack && slot != nullptr) {
        guard.ok = true;
        cache_->addref(slot);
        auto* cache = cache_.get();
        std::string path = ft.path;
        pool_->enqueue(Priority::kCont,
                       [this, cache, slot, path, bytes](WorkerCtx&) {
                         try {
                           write_file_atomic(path, slot->buf->host(), bytes);
                           stats_inc([](EngineStats& s) {
                             s.files_written++;
                             s.writeback_flushes++;
                           });
                         } catch (const std::exception& e) {
                           KVO_LOG_ERROR("writeback flush %s failed: %s",
                                         path.c_str(), e.what());
                           stats_inc([](EngineStats& s) { s.errors++; });
                         }
                         cache->release(slot);
                       });
        stats_inc([&](EngineStats& s) {
          s.bytes_stored += bytes;
          s.host_cache_stores++;
        });
        return false;
      }
    } else {
      // KV-ready fence: the gather must observe the serving engine's
      // completed KV writes for these blocks.
      double t0 = now_s();
      KVO_HIP_CHECK(hipStreamWaitEvent(ctx.stream, job->kv_ready, 0));
      uint8_t* kernel_dst = cfg_.copy_path == CopyPath::kStaged
                                ? ctx.device_staging->ptr()
                                : ctx.host_staging->device();
      const int32_t* ids_dev = stage_ids(ctx, ft);
      hipError_t err;
      if (cfg_.serialize == Serialize::kFp8E4M3Group) {
        // single-pass gather for the staged AND the zero-copy destination:
        // no scratch, so the tail of the device bounce goes unused
        err = kvc_launch_gather_fp8_group(
            const_cast<const void* const*>(dev_layer_ptrs_[ft.group]),
            dev_layer_strides_[ft.group], nl, g.block_bytes,
            cfg_.fp8_group_size, ft.block_ids.data(), nb, ids_dev, kernel_dst,
            ctx.stream, footer_bytes(), static_cast<int>(cfg_.kv_dtype));
      } else if (cfg_.serialize == Serialize::kFp4E2M1Group) {
        // the same single-pass shape, for both destinations
        err = kvc_launch_gather_fp4_group(
            const_cast<const void* const*>(dev_layer_ptrs_[ft.group]),
            dev_layer_strides_[ft.group], nl, g.block_bytes,
            cfg_.fp4_group_size, ft.block_ids.data(), nb, ids_dev, kernel_dst,
            ctx.stream, footer_bytes(), static_cast<int>(cfg_.kv_dtype));
      } else if (cfg_.serialize == Serialize::kFp8E4M3) {
        if (cfg_.copy_path == CopyPath::kStaged) {
          // split amax+quantize (chip-filling); the partial-max scratch
          // (tiles x slices floats, slices <= 2048/tiles + 1) lives in the
          // tail of the device bounce — packed fp8 is half of raw, so the
          // raw-sized bounce leaves bytes/1 >= tiles*slices*4 of room
          // (worst case 2048+tiles floats ~ 16 KiB)
          float* scratch = reinterpret_cast<float*>(
              ctx.device_staging->ptr() + bytes);
          err = kvc_launch_gather_fp8_split(
              const_cast<const void* const*>(dev_layer_ptrs_[ft.group]),
              dev_layer_strides_[ft.group], nl, g.block_bytes,
              ft.block_ids.data(), nb, ids_dev, kernel_dst, scratch,
              ctx.stream, footer_bytes(), static_cast<int>(cfg_.kv_dtype));
        } else {
          // zero-copy writes pinned host directly: atomics over PCIe are
          // pathological, keep the fused single-workgroup variant
          err = kvc_launch_gather_fp8(
              const_cast<const void* const*>(dev_layer_ptrs_[ft.group]),
              dev_layer_strides_[ft.group], nl, g.block_bytes,
              ft.block_ids.data(), nb, ids_dev, kernel_dst, ctx.stream,
              footer_bytes(), static_cast<int>(cfg_.kv_dtype));
        }
      } else {
        err = kvc_launch_gather(
            const_cast<const void* const*>(dev_layer_ptrs_[ft.group]),
            dev_layer_strides_[ft.group], nl, g.block_bytes,
            ft.block_ids.data(), nb, ids_dev, kernel_dst, ctx.stream,
            footer_bytes());
      }
      if (err != hipSuccess) throw HipError(hipGetErrorString(err));
      if (cfg_.checksum && cfg_.copy_path == CopyPath::kStaged) {
        // seal on the bounce, behind the gather and ahead of gather_done:
        // every staged branch below ships footers with its first D2H
        err = kvc_launch_seal_records(
            kernel_dst, static_cast<uint32_t>(nb) * nl, tile_payload_bytes(g),
            checksum_scratch(ctx, bytes), ctx.stream);
        if (err != hipSuccess) throw HipError(hipGetErrorString(err));
      }
      double t1 = now_s();
      stats_inc([&](EngineStats& s) { s.t_gather_ms += (t1 - t0) * 1e3; });
      if (cfg_.copy_path == CopyPath::kStaged &&
          cfg_.write_policy == WritePolicy::kBack && slot != nullptr) {
        // Write-back: the store completes once the slab is resident in
        // the DRAM tier; the file flush runs as a background task.
        hipEvent_t gather_done;
        KVO_HIP_CHECK(hipEventCreateWithFlags(&gather_done, hipEventDisableTiming));
        KVO_HIP_CHECK(hipEventRecord(gather_done, ctx.stream));
        double c0 = now_s();
        try {
          mover_->d2h(host_buf, ctx.device_staging->ptr(), bytes, gather_done);
        } catch (...) {
          (void)hipEventDestroy(gather_done);
          throw;
        }
        (void)hipEventDestroy(gather_done);
        double c1 = now_s();
        guard.ok = true;  // publish + release the store's reference
        cache_->addref(slot);
        auto* cache = cache_.get();
        std::string path = ft.path;
        pool_->enqueue(Priority::kCont,
                       [this, cache, slot, path, bytes](WorkerCtx&) {
                         double w0 = now_s();
                         try {
                           AtomicFileWriter w(path, cfg_.direct_io);
                           w.write_at(0, slot->buf->host(), bytes);
                           w.commit();
                           stats_inc([&](EngineStats& s) {
                             s.files_written++;
                             s.writeback_flushes++;
                             s.t_write_ms += (now_s() - w0) * 1e3;
                           });
                         } catch (const std::exception& e) {
                           KVO_LOG_ERROR("writeback flush %s failed: %s",
                                         path.c_str(), e.what());
                           stats_inc([](EngineStats& s) { s.errors++; });
                         }
                         cache->release(slot);
                       });
        stats_inc([&](EngineStats& s) {
          s.t_d2h_ms += (c1 - c0) * 1e3;
          s.bytes_stored += bytes;
          s.host_cache_stores++;
        });
        return false;
      }
      if (cfg_.copy_path == CopyPath::kStaged && slot != nullptr &&
          two_stage_stores()) {
        // Two-stage write-through store: this worker completes once the
        // D2H lands in the DRAM slot; the file write runs as its OWN task
        // (completion still waits for the rename — durability unchanged).
        // Per-worker serialization of [D2H -> write] left the D2H lane
        // idle whenever every worker sat in write(): the duplex wire
        // measures ~104 GB/s total (profiles/r02) while the bench ran
        // ~54 — the lane must stay fed from the next task's D2H. The
        // continuation runs in the kCont class: read-preferring workers
        // pick writes up after their loads drain while write-preferring
        // workers keep pumping store D2Hs (thread_pool.h preferences).
        hipEvent_t gather_done;
        KVO_HIP_CHECK(hipEventCreateWithFlags(&gather_done, hipEventDisableTiming));
        KVO_HIP_CHECK(hipEventRecord(gather_done, ctx.stream));
        double c0 = now_s();
        try {
          mover_->d2h(host_buf, ctx.device_staging->ptr(), bytes, gather_done);
        } catch (...) {
          (void)hipEventDestroy(gather_done);
          throw;
        }
        (void)hipEventDestroy(gather_done);
        double c1 = now_s();
        guard.ok = true;  // publish the slot; store's reference released
        cache_->addref(slot);
        auto* cache = cache_.get();
        std::string path = ft.path;
        pool_->enqueue(Priority::kCont,
                       [this, job, cache, slot, path, bytes](WorkerCtx&) {
          bool wok = true;
          if (!job->cancelled.load(std::memory_order_acquire)) {
            double w0 = now_s();
            try {
              AtomicFileWriter w(path, cfg_.direct_io);
              w.write_at(0, slot->buf->host(), bytes);
              w.commit();
              double dt = now_s() - w0;
              update_write_ema(dt);
              stats_inc([&](EngineStats& s) {
                s.files_written++;
                s.t_write_ms += dt * 1e3;
              });
            } catch (const std::exception& e) {
              KVO_LOG_ERROR("store write %s failed: %s", path.c_str(),
                            e.what());
              stats_inc([](EngineStats& s) { s.errors++; });
              wok = false;
            }
          } else {
            stats_inc([](EngineStats& s) { s.tasks_cancelled++; });
          }
          cache->release(slot);
          pending_writes_.fetch_sub(1, std::memory_order_relaxed);
          task_done(job, wok);
        });
        stats_inc([&](EngineStats& s) {
          s.t_d2h_ms += (c1 - c0) * 1e3;
          s.bytes_stored += bytes;
          s.host_cache_stores++;
        });
        return true;
      }
      if (cfg_.copy_path == CopyPath::kStaged) {
        // Chunked pipeline: D2H of chunk i+1 rides the SDMA mover while
        // chunk i is written to the file (zero CU occupancy on the wire;
        // one stream per direction saturates it — see pcie_mover.h).
        hipEvent_t gather_done;
        KVO_HIP_CHECK(hipEventCreateWithFlags(&gather_done, hipEventDisableTiming));
        KVO_HIP_CHECK(hipEventRecord(gather_done, ctx.stream));
        double t_copy = 0, t_io = 0;
        try {
          const size_t chunk = pipeline_chunk(bytes);
          AtomicFileWriter writer(ft.path, cfg_.direct_io);
          std::vector<std::future<void>> futs;
          for (size_t off = 0; off < bytes; off += chunk) {
            size_t n = std::min(chunk, bytes - off);
            futs.push_back(mover_->d2h_async(
                host_buf + off, ctx.device_staging->ptr() + off,
                n, off == 0 ? gather_done : nullptr));
          }
          size_t i = 0;
          for (size_t off = 0; off < bytes; off += chunk, ++i) {
            size_t n = std::min(chunk, bytes - off);
            double w0 = now_s();
            futs[i].get();
            double w1 = now_s();
            writer.write_at(off, host_buf + off, n);
            double w2 = now_s();
            t_copy += w1 - w0;
            t_io += w2 - w1;
          }
          writer.commit();
        } catch (...) {
          (void)hipEventDestroy(gather_done);
          throw;
        }
        (void)hipEventDestroy(gather_done);
        guard.ok = true;
        stats_inc([&](EngineStats& s) {
          s.t_d2h_ms += t_copy * 1e3;
          s.t_write_ms += t_io * 1e3;
          s.files_written++;
          s.bytes_stored += bytes;
          if (slot) s.host_cache_stores++;
        });
        return false;
      }
      KVO_HIP_CHECK(hipStreamSynchronize(ctx.stream));
      // zero-copy: the records already sit in pinned host memory; a device
      // pass would read them back across PCIe, so the host twin seals them
      if (cfg_.checksum)
        seal_records_host(host_buf, static_cast<size_t>(nb) * nl,
                          tile_payload_bytes(g));
      double t2 = now_s();
      stats_inc([&](EngineStats& s) { s.t_d2h_ms += (t2 - t1) * 1e3; });
    }
    double tw = now_s();
    write_file_atomic(ft.path, host_buf, bytes);
    double tw2 = now_s();
    guard.ok = true;
    stats_inc([&](EngineStats& s) {
      s.files_written++;
      s.bytes_stored += bytes;
      s.t_write_ms += (tw2 - tw) * 1e3;
      if (slot) s.host_cache_stores++;
    });
    return false;
  }

  // Scatter (raw), or dequantize+scatter (fp8 and fp4 modes), of the packed
  // records at `src` into the pages of ft.block_ids.
  hipError_t launch_scatter(WorkerCtx& ctx, const FileTransfer& ft,
                            const int32_t* ids_dev, const uint8_t* src) {
    const GroupDesc& g = groups_[ft.group];
    const int nb = static_cast<int>(ft.block_ids.size());
    const int nl = static_cast<int>(g.layer_ptrs.size());
    const void* const* ptrs =
        const_cast<const void* const*>(dev_layer_ptrs_[ft.group]);
    const uint64_t* strides = dev_layer_strides_[ft.group];
    switch (cfg_.serialize) {
      case Serialize::kFp8E4M3Group:
        return kvc_launch_scatter_fp8_group(
            ptrs, strides, nl, g.block_bytes, cfg_.fp8_group_size,
            ft.block_ids.data(), nb, ids_dev, src, ctx.stream,
            footer_bytes(), static_cast<int>(cfg_.kv_dtype));
      case Serialize::kFp4E2M1Group:
        return kvc_launch_scatter_fp4_group(
            ptrs, strides, nl, g.block_bytes, cfg_.fp4_group_size,
            ft.block_ids.data(), nb, ids_dev, src, ctx.stream,
            footer_bytes(), static_cast<int>(cfg_.kv_dtype));
      case Serialize::kFp8E4M3:
        return kvc_launch_scatter_fp8(ptrs, strides, nl, g.block_bytes,
                                      ft.block_ids.data(), nb, ids_dev, src,
                                      ctx.stream, footer_bytes(),
                                      static_cast<int>(cfg_.kv_dtype));
      default:
        return kvc_launch_scatter(ptrs, strides, nl, g.block_bytes,
                                  ft.block_ids.data(), nb, ids_dev, src,
                                  ctx.stream, footer_bytes());
    }
  }

  void load_one(WorkerCtx& ctx, const FileTransfer& ft) {
    const GroupDesc& g = groups_[ft.group];
    const int nb = static_cast<int>(ft.block_ids.size());
    const int nl = static_cast<int>(g.layer_ptrs.size());
    const size_t bytes = file_bytes(g, nb);
    const uint64_t offset =
        static_cast<uint64_t>(ft.slot_offset) * nl * tile_record_bytes(g);

    // (file coverage is validated on the miss paths — a pinned-DRAM cache
    // hit must serve even when the file was already evicted from disk)
    auto check_file_span = [&]() {
      int64_t fsz = file_size(ft.path);
      if (fsz < 0 || static_cast<uint64_t>(fsz) < offset + bytes)
        throw FileIoError("file " + ft.path + " does not cover requested span");
    };

    if (cfg_.copy_path == CopyPath::kStaged) {
      // Pinned-DRAM tier: a cache hit skips the filesystem read entirely —
      // the H2D streams straight from the resident slab.
      HostPinnedCache::Slot* hit = cache_ ? cache_->lookup(ft.path) : nullptr;
      if (hit && hit->bytes_used < offset + bytes) {
        cache_->release(hit);
        hit = nullptr;
      }
      HostPinnedCache::Slot* fill = nullptr;
      uint8_t* host_buf = ctx.host_staging->host();
      if (hit) {
        host_buf = hit->buf->host() + offset;
      } else if (cache_ && offset == 0) {
        // populate the tier on a miss (full-span loads only)
        fill = cache_->acquire(ft.path, bytes);
        if (fill) host_buf = fill->buf->host();
      }
      struct LoadGuard {
        HostPinnedCache* c;
        HostPinnedCache::Slot* hit;
        HostPinnedCache::Slot* fill;
        bool ok = false;
        ~LoadGuard() {
          if (!c) return;
          if (hit) c->release(hit);
          if (fill) {
            if (ok) {
              c->publish(fill);
              c->release(fill);
            } else {
              c->abandon(fill);
            }
          }
        }
      } lguard{cache_.get(), hit, fill};

      const size_t chunk = pipeline_chunk(bytes);
      double t_read = 0, t_h2d = 0;
      std::vector<std::future<void>> futs;
      if (hit) {
        futs.push_back(mover_->h2d_async(ctx.device_staging->ptr(), host_buf,
                                         bytes));
      } else {
        check_file_span();
        FileReader reader(ft.path, cfg_.direct_io);
        double r0 = now_s();
        for (size_t off = 0; off < bytes; off += chunk) {
          size_t n = std::min(chunk, bytes - off);
          reader.read_at(offset + off, host_buf + off, n);
          double r1 = now_s();
          t_read += r1 - r0;
          futs.push_back(mover_->h2d_async(ctx.device_staging->ptr() + off,
                                           host_buf + off, n));
          r0 = now_s();
        }
      }
      double h0 = now_s();
      for (auto& f : futs) f.get();
      t_h2d = now_s() - h0;
      if (cfg_.checksum) {
        // verify the whole span on the bounce and read the verdict BEFORE
        // the scatter is launched: a bad record must not reach a KV page
        const uint32_t tiles = static_cast<uint32_t>(nb) * nl;
        ctx.verify_result[0] = 0xffffffffu;  // overwritten by the kernel
        ctx.verify_result[1] = 0;
        hipError_t verr = kvc_launch_verify_records(
            ctx.device_staging->ptr(), tiles, tile_payload_bytes(g),
            checksum_scratch(ctx, bytes), ctx.verify_result_dev, ctx.stream);
        if (verr != hipSuccess) throw HipError(hipGetErrorString(verr));
        KVO_HIP_CHECK(hipStreamSynchronize(ctx.stream));
        const uint32_t bad = ctx.verify_result[0];
        if (bad != 0)
          checksum_failed(ft, nl, bad > tiles ? tiles : bad,
                          bad > tiles ? 0 : ctx.verify_result[1],
                          hit ? "DRAM-tier copy of" : "file");
      }
      touch_atime(ft.path);
      const int32_t* ids_dev = stage_ids(ctx, ft);
      hipError_t err =
          launch_scatter(ctx, ft, ids_dev, ctx.device_staging->ptr());
      if (err != hipSuccess) throw HipError(hipGetErrorString(err));
      double s0 = now_s();
      KVO_HIP_CHECK(hipStreamSynchronize(ctx.stream));
      double s1 = now_s();
      lguard.ok = true;
      stats_inc([&](EngineStats& s) {
        s.t_read_ms += t_read * 1e3;
        s.t_h2d_ms += t_h2d * 1e3;
        s.t_scatter_ms += (s1 - s0) * 1e3;
        s.files_read++;
        s.bytes_loaded += bytes;
        if (hit) s.host_cache_hits++;
      });
      return;
    }

    if (cfg_.copy_path == CopyPath::kHostMemcpy && cache_) {
      HostPinnedCache::Slot* hit = cache_->lookup(ft.path);
      if (hit && hit->bytes_used >= offset + bytes) {
        if (cfg_.checksum) {
          struct Release {
            HostPinnedCache* c;
            HostPinnedCache::Slot* s;
            ~Release() {
              if (s) c->release(s);
            }
          } rel{cache_.get(), hit};
          verify_host(ft, g, static_cast<size_t>(nb) * nl,
                      hit->buf->host() + offset, "DRAM-tier copy of");
          rel.s = nullptr;
        }
        scatter_host(g, ft.block_ids, hit->buf->host() + offset);
        touch_atime(ft.path);
        cache_->release(hit);
        stats_inc([&](EngineStats& s) {
          s.files_read++;
          s.bytes_loaded += bytes;
          s.host_cache_hits++;
        });
        return;
      }
      if (hit) cache_->release(hit);
    }
    check_file_span();
    double t0 = now_s();
    read_file_range(ft.path, offset, ctx.host_staging->host(), bytes);
    touch_atime(ft.path);
    double t1 = now_s();
    stats_inc([&](EngineStats& s) { s.t_read_ms += (t1 - t0) * 1e3; });
    // host and zero-copy: the span sits in host memory, the host twin checks
    // it before scatter_host / the scatter launch
    if (cfg_.checksum)
      verify_host(ft, g, static_cast<size_t>(nb) * nl,
                  ctx.host_staging->host(), "file");

    if (cfg_.copy_path == CopyPath::kHostMemcpy) {
      scatter_host(g, ft.block_ids, ctx.host_staging->host());
    } else {
      const uint8_t* kernel_src = ctx.host_staging->device();
      double t2 = now_s();
      stats_inc([&](EngineStats& s) { s.t_h2d_ms += (t2 - t1) * 1e3; });
      const int32_t* ids_dev = stage_ids(ctx, ft);
      hipError_t err = launch_scatter(ctx, ft, ids_dev, kernel_src);
      if (err != hipSuccess) throw HipError(hipGetErrorString(err));
      KVO_HIP_CHECK(hipStreamSynchronize(ctx.stream));
      double t3 = now_s();
      stats_inc([&](EngineStats& s) { s.t_scatter_ms += (t3 - t2) * 1e3; });
    }
    stats_inc([&](EngineStats& s) {
      s.files_read++;
      s.bytes_loaded += bytes;
    });
  }

  void gather_host(const GroupDesc& g, const std::vector<int32_t>& ids,
                   uint8_t* dst) const {
    const size_t nl = g.layer_ptrs.size();
    const size_t rec = tile_record_bytes(g);
    for (size_t bi = 0; bi < ids.size(); ++bi) {
      for (size_t l = 0; l < nl; ++l) {
        const uint8_t* src = static_cast<const uint8_t*>(g.layer_ptrs[l]) +
                             static_cast<uint64_t>(ids[bi]) * g.layer_strides[l];
        uint8_t* out = dst + (bi * nl + l) * rec;
        if (cfg_.serialize == Serialize::kFp8E4M3)
          fp8_quantize_tile(src, g.block_bytes, out, cfg_.kv_dtype);
        else if (cfg_.serialize == Serialize::kFp8E4M3Group)
          fp8_group_quantize_tile(src, g.block_bytes, cfg_.fp8_group_size, out,
                                  cfg_.kv_dtype);
        else if (cfg_.serialize == Serialize::kFp4E2M1Group)
          fp4_group_quantize_tile(src, g.block_bytes, cfg_.fp4_group_size, out,
                                  cfg_.kv_dtype);
        else
          std::memcpy(out, src, g.block_bytes);
      }
    }
  }

  void scatter_host(const GroupDesc& g, const std::vector<int32_t>& ids,
                    const uint8_t* src) const {
    const size_t nl = g.layer_ptrs.size();
    const size_t rec = tile_record_bytes(g);
    for (size_t bi = 0; bi < ids.size(); ++bi) {
      for (size_t l = 0; l < nl; ++l) {
        uint8_t* dst = static_cast<uint8_t*>(g.layer_ptrs[l]) +
                       static_cast<uint64_t>(ids[bi]) * g.layer_strides[l];
        const uint8_t* in = src + (bi * nl + l) * rec;
        if (cfg_.serialize == Serialize::kFp8E4M3)
          fp8_dequantize_tile(in, g.block_bytes, dst, cfg_.kv_dtype);
        else if (cfg_.serialize == Serialize::kFp8E4M3Group)
          fp8_group_dequantize_tile(in, g.block_bytes, cfg_.fp8_group_size, dst,
                                    cfg_.kv_dtype);
        else if (cfg_.serialize == Serialize::kFp4E2M1Group)
          fp4_group_dequantize_tile(in, g.block_bytes, cfg_.fp4_group_size, dst,
                                    cfg_.kv_dtype);
        else
          std::memcpy(dst, in, g.block_bytes);
      }
    }
  }

  // ---- software fp8 e4m3fn (host-mode twin of the CDNA4 kernels) -----------

  // Host twins of the kernels' page traits.
  struct PageBf16 {
    static float to_f32(uint16_t u) {
      uint32_t w = static_cast<uint32_t>(u) << 16;
      float f;
      std::memcpy(&f, &w, 4);
      return f;
    }
    static uint16_t from_f32(float f) {
      uint32_t w;
      std::memcpy(&w, &f, 4);
      uint32_t rounding = 0x7fff + ((w >> 16) & 1);
      return static_cast<uint16_t>((w + rounding) >> 16);
    }
  };
  // Portable IEEE binary16 bit conversions (no F16C): exact widening with
  // subnormals, and round-to-nearest-even narrowing that produces
  // subnormals and overflows to infinity from 65520 up.
  struct PageFp16 {
    static float to_f32(uint16_t u) {
      const uint32_t sign = static_cast<uint32_t>(u & 0x8000u) << 16;
      const uint32_t em = u & 0x7fffu;
      uint32_t w;
      float f;
      if (em >= 0x7c00u) {  // inf / NaN
        w = 0x7f800000u | ((em & 0x3ffu) << 13);
      } else if (em < 0x0400u) {  // zero / subnormal: em * 2^-24, exact
        f = static_cast<float>(em) * 5.9604644775390625e-08f;
        std::memcpy(&w, &f, 4);
      } else {
        w = (em << 13) + ((127u - 15u) << 23);
      }
      w |= sign;
      std::memcpy(&f, &w, 4);
      return f;
    }
    static uint16_t from_f32(float f) {
      uint32_t w;
      std::memcpy(&w, &f, 4);
      const uint32_t sign = (w >> 16) & 0x8000u;
      w &= 0x7fffffffu;
      uint32_t o;
      if (w >= ((127u + 16u) << 23)) {  // >= 65536, inf, NaN
        o = w > 0x7f800000u ? 0x7e00u : 0x7c00u;
      } else if (w < (113u << 23)) {
        // below the min normal 2^-14: the ulp of [0.5, 1) is 2^-24, the fp16
        // subnormal step, so adding 0.5 leaves RNE(|f| / 2^-24) in the low
        // mantissa bits (1024 = the encoding of 2^-14 itself)
        float a;
        std::memcpy(&a, &w, 4);
        a += 0.5f;
        std::memcpy(&o, &a, 4);
        o -= 0x3f000000u;
      } else {
        // rebias, then round the 13 dropped bits to even; a carry runs into
        // the exponent by itself (65520 and up become 0x7c00)
        const uint32_t odd = (w >> 13) & 1u;
        w += 0xc8000fffu + odd;  // ((15 - 127) << 23) + 0xfff, mod 2^32
        o = w >> 13;
      }
      return static_cast<uint16_t>(sign | o);
    }
  };
  // Round-to-nearest-even OCP e4m3fn encoder (1s 4e 3m, bias 7, max 448,
  // no inf) of both fp8 modes: the CDNA4 cvt_pk_fp8_f32 rounding, ties to
  // even, saturating at +-448. Finite inputs only (fp8_quantize_tile guards
  // NaN itself); the sign survives a magnitude that rounds to zero.
  // Branch-free, so the quantize loops vectorize and a tile of tiny scaled
  // values (amax = Inf makes every one of them 0) costs no more than any
  // other.
  static uint8_t f32_to_fp8_rne(float x) {
    uint32_t w;
    std::memcpy(&w, &x, 4);
    const uint32_t sign = (w >> 24) & 0x80u;
    w &= 0x7fffffffu;
    float a;
    std::memcpy(&a, &w, 4);
    // below the min normal 2^-6: code = RNE(a / 2^-9) in [0, 8]; 8 is the
    // encoding of 2^-6 itself. a * 512 is exact, and adding 1.5 * 2^23
    // leaves that integer, rounded to nearest even, in the low mantissa bits
    const float f = a * 512.0f + 12582912.0f;
    uint32_t sub;
    std::memcpy(&sub, &f, 4);
    sub &= 0xffu;
    // f32 bits >> 20 = (exponent << 3) | top-3 mantissa bits; rounding the
    // dropped 20 bits to even carries into the exponent by itself
    const uint32_t r = w + 0x7ffffu + ((w >> 20) & 1);
    uint32_t code = (r >> 20) - ((127u - 7u) << 3);
    code = code > 0x7eu ? 0x7eu : code;
    code = a < 0.015625f ? sub : code;
    return static_cast<uint8_t>(sign | code);
  }
  static float fp8_to_f32(uint8_t b) {
    uint8_t sign = b & 0x80;
    int exp_field = (b >> 3) & 0xf;
    int m = b & 0x7;
    if (exp_field == 0xf && m == 0x7) return NAN;
    float v;
    if (exp_field == 0)
      v = m * 0.001953125f;  // m * 2^-9
    else
      v = std::ldexp(1.0f + m / 8.0f, exp_field - 7);
    return sign ? -v : v;
  }

  // ---- software fp4 e2m1 (host twin of the fp4-group kernels) --------------
  // Round-to-nearest-even onto {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating, as
  // the compare chain that defines the format (the kernels use the gfx950
  // packed convert, which returns the same code for every finite f32). A
  // tie goes to the even code, so the thresholds alternate between > and
  // >=; the sign bit is copied whatever the magnitude rounds to. Finite
  // inputs only.
  static uint8_t f32_to_fp4_rne(float t) {
    uint32_t w;
    std::memcpy(&w, &t, 4);
    const float a = std::abs(t);
    const uint32_t mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) +
                         (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return static_cast<uint8_t>(((w >> 28) & 8u) | mag);
  }
  static float fp4_to_f32(uint8_t code) {
    static constexpr float kMag[8] = {0.0f, 0.5f, 1.0f, 1.5f,
                                      2.0f, 3.0f, 4.0f, 6.0f};
    const float m = kMag[code & 7];
    return (code & 8) ? -m : m;
  }

  public:
  // Shared software fp8 path (BlockCopier's host mode reuses it).
  // footer: bytes every record carries behind its payload (0 or 16).
  static void host_fp8_copy(const GroupDesc& g, const std::vector<int32_t>& ids,
                            uint8_t* packed, bool quantize, size_t footer = 0,
                            KvDtype kv_dtype = KvDtype::kBf16) {
    const size_t nl = g.layer_ptrs.size();
    const size_t rec = g.block_bytes / 2 + 4 + footer;
    for (size_t bi = 0; bi < ids.size(); ++bi) {
      for (size_t l = 0; l < nl; ++l) {
        uint8_t* page = static_cast<uint8_t*>(g.layer_ptrs[l]) +
                        static_cast<uint64_t>(ids[bi]) * g.layer_strides[l];
        uint8_t* slab = packed + (bi * nl + l) * rec;
        if (quantize)
          fp8_quantize_tile(page, g.block_bytes, slab, kv_dtype);
        else
          fp8_dequantize_tile(slab, g.block_bytes, page, kv_dtype);
      }
    }
  }

  static size_t fp8_group_record_bytes(uint64_t block_bytes, int group_size) {
    const size_t n = block_bytes / 2;
    return n + 4 * (n / static_cast<size_t>(group_size));
  }

  // Software twin of kvc_gather_fp8_group / kvc_scatter_fp8_group (engine
  // host mode and BlockCopier's CPU path): same bytes as the kernels.
  static void host_fp8_group_copy(const GroupDesc& g,
                                  const std::vector<int32_t>& ids,
                                  uint8_t* packed, int group_size,
                                  bool quantize, size_t footer = 0,
                                  KvDtype kv_dtype = KvDtype::kBf16) {
    const size_t nl = g.layer_ptrs.size();
    const size_t rec =
        fp8_group_record_bytes(g.block_bytes, group_size) + footer;
    for (size_t bi = 0; bi < ids.size(); ++bi) {
      for (size_t l = 0; l < nl; ++l) {
        uint8_t* page = static_cast<uint8_t*>(g.layer_ptrs[l]) +
                        static_cast<uint64_t>(ids[bi]) * g.layer_strides[l];
        uint8_t* slab = packed + (bi * nl + l) * rec;
        if (quantize)
          fp8_group_quantize_tile(page, g.block_bytes, group_size, slab,
                                  kv_dtype);
        else
          fp8_group_dequantize_tile(slab, g.block_bytes, group_size, page,
                                    kv_dtype);
      }
    }
  }

  static size_t fp4_group_record_bytes(uint64_t block_bytes, int group_size,
                                       KvDtype kv_dtype = KvDtype::kBf16) {
    const size_t n = kv_tile_elems(block_bytes, kv_dtype);
    return n / 2 + 4 * (n / static_cast<size_t>(group_size));
  }

  // Software twin of kvc_gather_fp4_group / kvc_scatter_fp4_group (engine
  // host mode and BlockCopier's CPU path): same bytes as the kernels.
  static void host_fp4_group_copy(const GroupDesc& g,
                                  const std::vector<int32_t>& ids,
                                  uint8_t* packed, int group_size,
                                  bool quantize, size_t footer = 0,
                                  KvDtype kv_dtype = KvDtype::kBf16) {
    const size_t nl = g.layer_ptrs.size();
    const size_t rec =
        fp4_group_record_bytes(g.block_bytes, group_size, kv_dtype) + footer;
    for (size_t bi = 0; bi < ids.size(); ++bi) {
      for (size_t l = 0; l < nl; ++l) {
        uint8_t* page = static_cast<uint8_t*>(g.layer_ptrs[l]) +
                        static_cast<uint64_t>(ids[bi]) * g.layer_strides[l];
        uint8_t* slab = packed + (bi * nl + l) * rec;
        if (quantize)
          fp4_group_quantize_tile(page, g.block_bytes, group_size, slab,
                                  kv_dtype);
        else
          fp4_group_dequantize_tile(slab, g.block_bytes, group_size, page,
                                    kv_dtype);
      }
    }
  }

  private:
  // Record starts are only 4-byte aligned and scales follow n payload
  // bytes: scales move through memcpy.
  template <typename T>
  static void fp8_group_quantize_tile_t(const uint8_t* src, size_t block_bytes,
                                      int group_size, uint8_t* out) {
    const size_t n = block_bytes / 2;
    const size_t G = static_cast<size_t>(group_size);
    const uint16_t* in = reinterpret_cast<const uint16_t*>(src);
    for (size_t gi = 0; gi < n / G; ++gi) {
      const uint16_t* x = in + gi * G;
      float amax = 0.0f;
      for (size_t i = 0; i < G; ++i)
        amax = std::max(amax, std::abs(T::to_f32(x[i])));
      if (amax <= 0.0f) amax = 1.0f;
      const float scale = amax / 448.0f;
      const float inv = 448.0f / amax;
      for (size_t i = 0; i < G; ++i)
        out[gi * G + i] = f32_to_fp8_rne(T::to_f32(x[i]) * inv);
      std::memcpy(out + n + 4 * gi, &scale, 4);
    }
  }

  template <typename T>
  static void fp8_group_dequantize_tile_t(const uint8_t* in, size_t block_bytes,
                                        int group_size, uint8_t* dst) {
    const size_t n = block_bytes / 2;
    const size_t G = static_cast<size_t>(group_size);
    uint16_t* out = reinterpret_cast<uint16_t*>(dst);
    for (size_t gi = 0; gi < n / G; ++gi) {
      float scale;
      std::memcpy(&scale, in + n + 4 * gi, 4);
      for (size_t i = 0; i < G; ++i)
        out[gi * G + i] = T::from_f32(fp8_to_f32(in[gi * G + i]) * scale);
    }
  }

  // fp4: G is even, so a group starts on a byte boundary. The product
  // f32(value) * scale is rounded to f32 first and T::from_f32 then rounds
  // those bits to the page type in integer arithmetic: the two roundings of
  // the spec, for fp16 as for bf16 (one rounding differs for fp16
  // subnormal results; see fp4_page_from_product in kernels.hip).
  template <typename T>
  static void fp4_group_quantize_tile_t(const uint8_t* src, size_t block_bytes,
                                        int group_size, uint8_t* out) {
    const size_t n = block_bytes / 2;
    const size_t G = static_cast<size_t>(group_size);
    const uint16_t* in = reinterpret_cast<const uint16_t*>(src);
    for (size_t gi = 0; gi < n / G; ++gi) {
      const uint16_t* x = in + gi * G;
      float amax = 0.0f;
      for (size_t i = 0; i < G; ++i)
        amax = std::max(amax, std::abs(T::to_f32(x[i])));
      if (amax <= 0.0f) amax = 1.0f;
      const float scale = amax / 6.0f;
      const float inv = 6.0f / amax;
      uint8_t* codes = out + gi * G / 2;
      for (size_t i = 0; i < G; i += 2)
        codes[i / 2] = static_cast<uint8_t>(
            f32_to_fp4_rne(T::to_f32(x[i]) * inv) |
            (f32_to_fp4_rne(T::to_f32(x[i + 1]) * inv) << 4));
      std::memcpy(out + n / 2 + 4 * gi, &scale, 4);
    }
  }

  template <typename T>
  static void fp4_group_dequantize_tile_t(const uint8_t* in, size_t block_bytes,
                                          int group_size, uint8_t* dst) {
    const size_t n = block_bytes / 2;
    const size_t G = static_cast<size_t>(group_size);
    uint16_t* out = reinterpret_cast<uint16_t*>(dst);
    for (size_t gi = 0; gi < n / G; ++gi) {
      float scale;
      std::memcpy(&scale, in + n / 2 + 4 * gi, 4);
      const uint8_t* codes = in + gi * G / 2;
      for (size_t i = 0; i < G; i += 2) {
        out[gi * G + i] = T::from_f32(fp4_to_f32(codes[i / 2] & 0xf) * scale);
        out[gi * G + i + 1] =
            T::from_f32(fp4_to_f32(codes[i / 2] >> 4) * scale);
      }
    }
  }

  // fp4 over fp8 (e4m3fn) pages: n = block_bytes elements of one byte each.
  // Same arithmetic with x = the exact f32 value of the page byte; the load
  // rounds the f32 product to e4m3fn with f32_to_fp8_rne, which keeps
  // subnormals and copies the sign onto a zero magnitude (0x80). NaN page
  // bytes are out of scope (fmax drops them from amax, as the kernel's
  // fmaxf does).
  static void fp4_group_quantize_tile_fp8page(const uint8_t* src,
                                              size_t block_bytes,
                                              int group_size, uint8_t* out) {
    const size_t n = block_bytes;
    const size_t G = static_cast<size_t>(group_size);
    for (size_t gi = 0; gi < n / G; ++gi) {
      const uint8_t* x = src + gi * G;
      float amax = 0.0f;
      for (size_t i = 0; i < G; ++i)
        amax = std::max(amax, std::abs(fp8_to_f32(x[i])));
      if (amax <= 0.0f) amax = 1.0f;
      const float scale = amax / 6.0f;
      const float inv = 6.0f / amax;
      uint8_t* codes = out + gi * G / 2;
      for (size_t i = 0; i < G; i += 2)
        codes[i / 2] = static_cast<uint8_t>(
            f32_to_fp4_rne(fp8_to_f32(x[i]) * inv) |
            (f32_to_fp4_rne(fp8_to_f32(x[i + 1]) * inv) << 4));
      std::memcpy(out + n / 2 + 4 * gi, &scale, 4);
    }
  }

  static void fp4_group_dequantize_tile_fp8page(const uint8_t* in,
                                                size_t block_bytes,
                                                int group_size, uint8_t* dst) {
    const size_t n = block_bytes;
    const size_t G = static_cast<size_t>(group_size);
    for (size_t gi = 0; gi < n / G; ++gi) {
      float scale;
      std::memcpy(&scale, in + n / 2 + 4 * gi, 4);
      const uint8_t* codes = in + gi * G / 2;
      for (size_t i = 0; i < G; i += 2) {
        const float p0 = fp4_to_f32(codes[i / 2] & 0xf) * scale;
        const float p1 = fp4_to_f32(codes[i / 2] >> 4) * scale;
        dst[gi * G + i] = f32_to_fp8_rne(p0);
        dst[gi * G + i + 1] = f32_to_fp8_rne(p1);
      }
    }
  }

  template <typename T>
  static void fp8_quantize_tile_t(const uint8_t* src, size_t block_bytes,
                         uint8_t* out) {
    const size_t n = block_bytes / 2;
    const uint16_t* in = reinterpret_cast<const uint16_t*>(src);
    float amax = 0.0f;
    for (size_t i = 0; i < n; ++i)
      amax = std::max(amax, std::abs(T::to_f32(in[i])));
    if (amax <= 0.0f) amax = 1.0f;
    float scale = amax / 448.0f;
    float inv = 448.0f / amax;
    for (size_t i = 0; i < n; ++i) {
      const float x = T::to_f32(in[i]) * inv;
      // a NaN never enters amax (std::max keeps the other operand) and is
      // stored as the e4m3fn NaN code, so it loads as NaN
      out[i] = x != x ? 0x7f : f32_to_fp8_rne(x);
    }
    std::memcpy(out + n, &scale, 4);
  }

  template <typename T>
  static void fp8_dequantize_tile_t(const uint8_t* in, size_t block_bytes,
                           uint8_t* dst) {
    const size_t n = block_bytes / 2;
    float scale;
    std::memcpy(&scale, in + n, 4);
    uint16_t* out = reinterpret_cast<uint16_t*>(dst);
    for (size_t i = 0; i < n; ++i)
      out[i] = T::from_f32(fp8_to_f32(in[i]) * scale);
  }

  // Runtime page format -> the templated codec above.
  static void fp8_group_quantize_tile(const uint8_t* src, size_t block_bytes,
                                      int group_size, uint8_t* out,
                                      KvDtype kv_dtype) {
    if (kv_dtype == KvDtype::kFp16)
      fp8_group_quantize_tile_t<PageFp16>(src, block_bytes, group_size, out);
    else
      fp8_group_quantize_tile_t<PageBf16>(src, block_bytes, group_size, out);
  }
  static void fp8_group_dequantize_tile(const uint8_t* in, size_t block_bytes,
                                        int group_size, uint8_t* dst,
                                        KvDtype kv_dtype) {
    if (kv_dtype == KvDtype::kFp16)
      fp8_group_dequantize_tile_t<PageFp16>(in, block_bytes, group_size, dst);
    else
      fp8_group_dequantize_tile_t<PageBf16>(in, block_bytes, group_size, dst);
  }
  static void fp4_group_quantize_tile(const uint8_t* src, size_t block_bytes,
                                      int group_size, uint8_t* out,
                                      KvDtype kv_dtype) {
    if (kv_dtype == KvDtype::kFp8E4M3)
      fp4_group_quantize_tile_fp8page(src, block_bytes, group_size, out);
    else if (kv_dtype == KvDtype::kFp16)
      fp4_group_quantize_tile_t<PageFp16>(src, block_bytes, group_size, out);
    else
      fp4_group_quantize_tile_t<PageBf16>(src, block_bytes, group_size, out);
  }
  static void fp4_group_dequantize_tile(const uint8_t* in, size_t block_bytes,
                                        int group_size, uint8_t* dst,
                                        KvDtype kv_dtype) {
    if (kv_dtype == KvDtype::kFp8E4M3)
      fp4_group_dequantize_tile_fp8page(in, block_bytes, group_size, dst);
    else if (kv_dtype == KvDtype::kFp16)
      fp4_group_dequantize_tile_t<PageFp16>(in, block_bytes, group_size, dst);
    else
      fp4_group_dequantize_tile_t<PageBf16>(in, block_bytes, group_size, dst);
  }
  static void fp8_quantize_tile(const uint8_t* src, size_t block_bytes,
                                uint8_t* out, KvDtype kv_dtype) {
    if (kv_dtype == KvDtype::kFp16)
      fp8_quantize_tile_t<PageFp16>(src, block_bytes, out);
    else
      fp8_quantize_tile_t<PageBf16>(src, block_bytes, out);
  }
  static void fp8_dequantize_tile(const uint8_t* in, size_t block_bytes,
                                  uint8_t* dst, KvDtype kv_dtype) {
    if (kv_dtype == KvDtype::kFp16)
      fp8_dequantize_tile_t<PageFp16>(in, block_bytes, dst);
    else
      fp8_dequantize_tile_t<PageBf16>(in, block_bytes, dst);
  }

  EngineConfig cfg_;
  std::vector<GroupDesc> groups_;
  std::vector<void**> dev_layer_ptrs_;
  std::vector<uint64_t*> dev_layer_strides_;
  std::unique_ptr<IoThreadPool> pool_;
  std::unique_ptr<PcieMover> mover_;
  std::unique_ptr<HostPinnedCache> cache_;

  std::mutex jobs_mu_;  // guards jobs_/finished_/next_job_id_ only
  std::condition_variable done_cv_;
  std::unordered_map<int64_t, std::shared_ptr<Job>> jobs_;
  std::vector<FinishedJob> finished_;
  int64_t next_job_id_ = 1;
  std::atomic<size_t> pending_writes_{0};
  std::array<StatsShard, kStatsShards> stats_shards_;
  std::atomic<uint64_t> write_ema_bits_{0};  // double bit-pattern (0.0 = unset)
};

}  // namespace kvo
