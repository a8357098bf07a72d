// NUMA-pinned async I/O thread pool with read-priority QoS.
//
// Capability parity with the reference ThreadPool
// (csrc/storage/thread_pool.cpp): two priority classes (HIGH = loads,
// NORMAL = stores), a configurable fraction of read-preferring workers,
// work stealing across classes, per-worker HIP stream + pinned host staging
// + HBM bounce buffer, worker threads pinned round-robin to the CPUs of the
// GPU's NUMA node. Re-designed around std::function tasks that receive the
// worker context (no futures on the hot path — completion is job-counter
// based in the engine).
#pragma once

#include <numa.h>
#include <pthread.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"

namespace kvo {

struct WorkerCtx {
  int worker_id = -1;
  hipStream_t stream = nullptr;           // null in host mode
  HostStaging* host_staging = nullptr;    // pinned (GPU mode) or aligned malloc
  DeviceStaging* device_staging = nullptr;  // HBM bounce; empty in host mode
  int32_t* dev_ids = nullptr;  // device block-id buffer (> kernarg-limit paths)
  // Verdict of kvc_verify_records (bad count, first bad index): two words of
  // mapped pinned memory the kernel writes and the worker reads after its
  // stream sync. Null unless the engine verifies checksums on the bounce.
  volatile uint32_t* verify_result = nullptr;
  uint32_t* verify_result_dev = nullptr;
};

// kHigh = loads, kNormal = store front halves (gather + D2H), kCont =
// continuation work (the file-write half of a two-stage store, write-back
// flushes). Worker preference is asymmetric so the PCIe lanes stay fed:
//   read-preferring:  high -> cont -> normal   (loads, then writes)
//   write-preferring: normal -> cont -> high   (keep pumping D2Hs)
// A writer picking cont before normal would drain the D2H queue dry
// (measured: both lanes <50% busy at full wire speed per byte).
enum class Priority { kHigh = 0, kNormal = 1, kCont = 2 };

class IoThreadPool {
 public:
  using Task = std::function<void(WorkerCtx&)>;

  IoThreadPool(int n_threads, bool gpu_mode, int device, size_t host_staging_bytes,
               size_t device_staging_bytes, double read_preferring_ratio,
               bool mapped_host_staging = false, bool verify_result = false)
      : gpu_mode_(gpu_mode), device_(device),
        host_staging_bytes_(host_staging_bytes),
        device_staging_bytes_(device_staging_bytes),
        mapped_host_staging_(mapped_host_staging),
        verify_result_(verify_result) {
    n_threads = std::max(1, n_threads);
    int numa_node = -1;
    if (gpu_mode_) {
      numa_node = gpu_numa_node(device_);
      cpus_ = numa_node_cpus(numa_node);
      KVO_LOG_INFO("io pool: %d threads, gpu %d, numa node %d (%zu cpus)",
                   n_threads, device_, numa_node, cpus_.size());
    }
    numa_node_ = numa_node;
    int n_read_pref = static_cast<int>(n_threads * read_preferring_ratio + 0.5);
    ready_.resize(n_threads, 0);
    for (int i = 0; i < n_threads; ++i)
      workers_.emplace_back([this, i, n_read_pref] { run(i, i < n_read_pref); });
    // Wait for staging allocation so construction failures surface here.
    {
      std::unique_lock<std::mutex> g(mu_);
      started_cv_.wait(g, [this] {
        for (auto r : ready_)
          if (!r) return false;
        return true;
      });
      if (!init_error_.empty()) {
        g.unlock();
        shutdown();
        throw HipError(init_error_);
      }
    }
  }

  ~IoThreadPool() { shutdown(); }

  void enqueue(Priority prio, Task task) {
    {
      std::lock_guard<std::mutex> g(mu_);
      queue_for(prio).push_back(std::move(task));
    }
    cv_.notify_one();
  }

  size_t queued(Priority prio) {
    std::lock_guard<std::mutex> g(mu_);
    return queue_for(prio).size();
  }

  void shutdown() {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (stopping_) return;
      stopping_ = true;
    }
    cv_.notify_all();
    for (auto& w : workers_) w.join();
    workers_.clear();
  }

  int size() const { return static_cast<int>(workers_.size()); }

 private:
  void pin_to_numa(int i) {
    if (cpus_.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    CPU_SET(cpus_[i % cpus_.size()], &set);
    pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
    if (numa_node_ >= 0 && numa_available() >= 0)
      numa_set_preferred(numa_node_);
  }

  void run(int i, bool read_preferring) {
    WorkerCtx ctx;
    ctx.worker_id = i;
    std::unique_ptr<HostStaging> host_staging;
    std::unique_ptr<DeviceStaging> device_staging;
    std::unique_ptr<HostStaging> verify_result;
    try {
      if (gpu_mode_) {
        KVO_HIP_CHECK(hipSetDevice(device_));
        pin_to_numa(i);
        KVO_HIP_CHECK(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
        // 16 KiB: block-id staging for transfers above the kernarg limit
        KVO_HIP_CHECK(hipMalloc(&ctx.dev_ids, 4096 * sizeof(int32_t)));
      }
      host_staging = std::make_unique<HostStaging>(host_staging_bytes_, gpu_mode_,
                                                   mapped_host_staging_);
      device_staging =
          std::make_unique<DeviceStaging>(device_staging_bytes_, gpu_mode_);
      ctx.host_staging = host_staging.get();
      ctx.device_staging = device_staging.get();
      if (gpu_mode_ && verify_result_) {
        verify_result = std::make_unique<HostStaging>(64, true, /*mapped=*/true);
        ctx.verify_result = reinterpret_cast<uint32_t*>(verify_result->host());
        ctx.verify_result_dev =
            reinterpret_cast<uint32_t*>(verify_result->device());
      }
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> g(mu_);
      init_error_ = e.what();
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      ready_[i] = 1;
    }
    started_cv_.notify_all();

    std::deque<Task>* order[3];
    if (read_preferring) {
      order[0] = &high_;
      order[1] = &cont_;
      order[2] = &normal_;
    } else {
      order[0] = &normal_;
      order[1] = &cont_;
      order[2] = &high_;
    }
    for (;;) {
      Task task;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [this] {
          return stopping_ || !high_.empty() || !normal_.empty() ||
                 !cont_.empty();
        });
        std::deque<Task>* q = nullptr;
        for (auto* cand : order)
          if (!cand->empty()) {
            q = cand;
            break;
          }
        if (q == nullptr) break;  // stopping and drained
        task = std::move(q->front());
        q->pop_front();
      }
      try {
        task(ctx);
      } catch (const std::exception& e) {
        KVO_LOG_ERROR("io task failed: %s", e.what());
      }
    }
    if (ctx.dev_ids) (void)hipFree(ctx.dev_ids);
    if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
  }

  bool gpu_mode_;
  int device_;
  int numa_node_ = -1;
  size_t host_staging_bytes_;
  size_t device_staging_bytes_;
  bool mapped_host_staging_ = false;
  bool verify_result_ = false;
  std::vector<int> cpus_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::condition_variable started_cv_;
  std::deque<Task>& queue_for(Priority p) {
    return p == Priority::kHigh ? high_
                                : (p == Priority::kNormal ? normal_ : cont_);
  }

  std::deque<Task> high_, normal_, cont_;
  std::vector<std::thread> workers_;
  std::vector<char> ready_;
  std::string init_error_;
  bool stopping_ = false;
};

}  // namespace kvo
