// abi.hip — extern "C" entry points of include/relearn_hip.h, part: the allocator behind every handle, profiling, the
// engine and the collectives.  (Environments: abi_env.hip; modules: abi_module.hip; trajectories and rl_rollout:
// abi_traj.hip.)
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>

#include "abi_internal.hpp"

thread_local std::string g_last_error_no_engine;

// ---------------------------------------------------------------- the allocator behind DevMem (dev_mem.hpp)
// live device bytes and allocations of the whole process: what rl_debug_device_memory reads
static std::atomic<uint64_t> g_device_bytes{0}, g_device_allocations{0};

void *rl_device_alloc(uint64_t bytes) {
  void *p = nullptr;
  RL_HIP_CHECK(hipMalloc(&p, bytes));
  g_device_bytes += bytes;
  g_device_allocations += 1;
  return p;
}

void rl_device_free(void *p, uint64_t bytes) {
  (void)hipFree(p);
  g_device_bytes -= bytes;
  g_device_allocations -= 1;
}

void *rl_host_alloc(uint64_t bytes, bool mapped) {
  void *p = nullptr;
  RL_HIP_CHECK(hipHostMalloc(&p, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault));
  return p;
}

void rl_host_free(void *p) { (void)hipHostFree(p); }

// ---------------------------------------------------------------- profiling scope
ProfScope::ProfScope(rl_engine *eng, int c) : e(eng), cls(c) {
  if (!e->profiling) return;
  auto get = [&]() {
    hipEvent_t ev;
    if (!e->prof_event_pool.empty()) {
      ev = e->prof_event_pool.back();
      e->prof_event_pool.pop_back();
    } else if (hipEventCreate(&ev) != hipSuccess) {
      ev = nullptr;
    }
    return ev;
  };
  a = get();
  b = get();
  if (a) (void)hipEventRecord(a, e->stream);
}

ProfScope::~ProfScope() {
  if (!e->profiling || !a || !b) return;
  (void)hipEventRecord(b, e->stream);
  e->prof_pending.push_back({cls, {a, b}});
}

static void prof_drain(rl_engine *e) {
  for (auto &it : e->prof_pending) {
    float ms = 0.0f;
    (void)hipEventSynchronize(it.second.second);
    if (hipEventElapsedTime(&ms, it.second.first, it.second.second) == hipSuccess) {
      e->prof_ms[it.first] += (double)ms;
      e->prof_launches[it.first] += 1;
    }
    e->prof_event_pool.push_back(it.second.first);
    e->prof_event_pool.push_back(it.second.second);
  }
  e->prof_pending.clear();
}

// ---------------------------------------------------------------- RCCL through dlopen
// The library must load (and export every symbol) on machines without a GPU or without RCCL, and must not
// clash with an RCCL copy a host program (e.g. PyTorch) already mapped; so RCCL is bound at rl_comm_init.
namespace {
struct Rccl {
  void *handle = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, const void * /*ncclUniqueId by value: 128 bytes*/, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
struct UniqueId { char bytes[128]; };
typedef int (*comm_init_rank_t)(void **, int, UniqueId, int);

void rccl_load() {
  if (g_rccl.handle) return;
  // RCCL must run on the SAME HIP runtime as this library: a host program may have mapped a second copy of the ROCm
  // libraries (PyTorch bundles libamdhip64 / librccl under torch/lib), and a communicator created by the other copy's
  // RCCL cannot use this runtime's streams ("unhandled cuda error").  So: first the librccl that sits next to the
  // libamdhip64 this library is bound to, then the usual names.
  std::vector<std::string> names;
  Dl_info info;
  if (dladdr((void *)&hipGetDeviceCount, &info) != 0 && info.dli_fname != nullptr) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) {
      dir.resize(slash);
      names.push_back(dir + "/librccl.so.1");
      names.push_back(dir + "/librccl.so");
    }
  }
  names.push_back("librccl.so.1");
  names.push_back("librccl.so");
  names.push_back("/opt/rocm/lib/librccl.so.1");
  for (const std::string &n : names) {
    g_rccl.handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (g_rccl.handle) break;
  }
  if (!g_rccl.handle) throw RlError(RL_ERR_COMM, std::string("cannot dlopen librccl: ") + dlerror());
  g_rccl.GetUniqueId = (int (*)(void *))dlsym(g_rccl.handle, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void **, int, const void *, int))dlsym(g_rccl.handle, "ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(void *))dlsym(g_rccl.handle, "ncclCommDestroy");
  g_rccl.AllReduce =
      (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(g_rccl.handle, "ncclAllReduce");
  g_rccl.GetErrorString = (const char *(*)(int))dlsym(g_rccl.handle, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce)
    throw RlError(RL_ERR_COMM, "librccl is missing expected symbols");
}

void rccl_check(int rc, const char *what) {
  if (rc != 0)
    throw RlError(RL_ERR_COMM, std::string(what) + ": " +
                                   (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : std::to_string(rc).c_str()));
}
}  // namespace

// ---------------------------------------------------------------- in-process loopback collective
// RELEARN_LOOPBACK_COMM=1: rl_comm_init joins the engines of ONE process that present the same unique id into a
// group whose all-reduce is a kernel summing the ranks' buffers in rank order (all engines on the same GPU, each
// driven by its own host thread).  It exists so that the multi-rank arithmetic — lane sharding by global lane id,
// sample-weighted means over all ranks, identical redundant updates — can be exercised on a one-GPU box; the RCCL
// call path itself is exercised with a one-rank communicator (RELEARN_FORCE_RCCL=1).
// (`bad_rank` >= 0: a test of the tests — that rank's vector enters the sum multiplied by `bad_weight`, what a rank that
// weighs its samples by a wrong B_local / B_total contributes; every rank still receives the same sums, so the job runs
// to its end and must FAIL the sharded parity bars: tests/test_gpu_multirank.py, RELEARN_LOOPBACK_TEST_WEIGHT)
// (RELEARN_LOOPBACK_TIMEOUT_MS, read like the weight when the group is made: the deadline of one barrier wait, 120 s by
// default: tests/test_gpu_sharded_modules.py)
__global__ void k_loopback_sum(float *const *bufs, int n_ranks, size_t count, int bad_rank, float bad_weight) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float s = bad_rank == 0 ? bad_weight * bufs[0][i] : bufs[0][i];
  for (int r = 1; r < n_ranks; ++r) s = s + (r == bad_rank ? bad_weight * bufs[r][i] : bufs[r][i]);
  for (int r = 0; r < n_ranks; ++r) bufs[r][i] = s;
}

struct LoopbackGroup {
  std::mutex mu;
  std::condition_variable cv;
  int n_ranks = 0, arrived = 0, joined = 0;
  uint64_t generation = 0;
  std::vector<float *> bufs;
  float **d_bufs = nullptr;
  int bad_rank = -1;        // RELEARN_LOOPBACK_TEST_WEIGHT="rank:weight" when the group was made (k_loopback_sum)
  float bad_weight = 1.0f;  // ... applied to the gradient-sized vectors only (the set-up's rank count stays a count)
  // A rank that never arrives (it raised, or returned early) must not strand its peers' host threads: a wait ends after
  // `deadline` (RELEARN_LOOPBACK_TIMEOUT_MS when the group was made), the group is then failed for good, and every rank
  // that is in a barrier or enters one later gets RL_ERR_COMM.  (Host side only: a waiting rank has synchronised its
  // stream before it waits, no kernel is in flight.)
  std::chrono::milliseconds deadline{120000};
  bool failed = false;
  void barrier(std::unique_lock<std::mutex> &lk) {
    if (failed) throw RlError(RL_ERR_COMM, "loopback collective: a peer did not arrive");
    const uint64_t gen = generation;
    if (++arrived == n_ranks) {
      arrived = 0;
      generation += 1;
      cv.notify_all();
      return;
    }
    if (!cv.wait_for(lk, deadline, [&] { return generation != gen || failed; })) {
      failed = true;
      cv.notify_all();
    }
    if (generation == gen) throw RlError(RL_ERR_COMM, "loopback collective: a peer did not arrive");
  }
};
static std::mutex g_loopback_mu;
static std::map<std::string, std::shared_ptr<LoopbackGroup>> g_loopback_groups;

static void loopback_allreduce(rl_engine *e, float *d_buf, size_t count) {
  LoopbackGroup *g = e->loopback;
  RL_HIP_CHECK(hipStreamSynchronize(e->stream));  // this rank's contribution is complete
  std::unique_lock<std::mutex> lk(g->mu);
  g->bufs[e->rank] = d_buf;
  g->barrier(lk);
  if (e->rank == 0) {
    RL_HIP_CHECK(hipMemcpyAsync(g->d_bufs, g->bufs.data(), g->n_ranks * sizeof(float *), hipMemcpyHostToDevice,
                                e->stream));
    hipLaunchKernelGGL(k_loopback_sum, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->stream, g->d_bufs,
                       g->n_ranks, count, count > 64 ? g->bad_rank : -1, g->bad_weight);
    RL_HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  g->barrier(lk);
}

void rl_allreduce_sum_f32(rl_engine *e, float *d_buf, size_t count) {
  if (e->ipc_active) {
    if (!ipc_allreduce_fits(e, count))
      throw RlError(RL_ERR_UNSUPPORTED, "the peer-mailbox collective carries vectors of <= 2048 floats (feed-forward "
                                        "modules); use the RCCL transport for larger ones");
    ProfScope ps(e, RL_K_ALLREDUCE);
    ipc_allreduce(e, d_buf, count);
    return;
  }
  if (e->loopback) {
    ProfScope ps(e, RL_K_ALLREDUCE);
    loopback_allreduce(e, d_buf, count);
    return;
  }
  if (e->host_allreduce) {
    ProfScope ps(e, RL_K_ALLREDUCE);
    e->host_allreduce_buf.resize(count);
    RL_HIP_CHECK(hipMemcpyAsync(e->host_allreduce_buf.data(), d_buf, count * sizeof(float), hipMemcpyDeviceToHost,
                                e->stream));
    RL_HIP_CHECK(hipStreamSynchronize(e->stream));
    if (e->host_allreduce(e->host_allreduce_ctx, e->host_allreduce_buf.data(), count) != 0)
      throw RlError(RL_ERR_COMM, "the host all-reduce callback failed");
    RL_HIP_CHECK(hipMemcpyAsync(d_buf, e->host_allreduce_buf.data(), count * sizeof(float), hipMemcpyHostToDevice,
                                e->stream));
    RL_HIP_CHECK(hipStreamSynchronize(e->stream));
    return;
  }
  if (!e->comm) {
    // several ranks and nothing to exchange with: every update would scale by the global sample count while summing
    // local samples only, and the replicas would drift apart silently
    if (e->n_ranks > 1) throw RlError(RL_ERR_COMM, "engine has n_ranks > 1 but no collective (rl_comm_init failed?)");
    return;
  }
  ProfScope ps(e, RL_K_ALLREDUCE);
  // ncclFloat32 = 7, ncclSum = 0
  // (the auxiliary chain has a communicator of its own: collectives of two chains in flight on two streams must not
  // share one — rl_actor_critic_update runs the chains one after the other when there is no second communicator)
  void *comm = e->chan == 1 && e->comm_aux ? e->comm_aux : e->comm;
  rccl_check(g_rccl.AllReduce(d_buf, d_buf, count, 7, 0, comm, e->stream), "ncclAllReduce");
}

// Settings every rank has to take the same way, decided through the collective that was just installed: an all-reduce
// that also counts the ranks (a transport that does not reach everybody fails here, not in the first update).
//   RELEARN_SERIAL_UPDATE in ANY rank's environment -> the update chains run in turn on EVERY rank (a rank running them
//   side by side would put the critic's collectives on the auxiliary channel, its peers on the main one).
// rl_engine_set_serial_update is an API call, not an environment: the host program makes it on every rank or on none.
void comm_agree(rl_engine *e) {
  const bool mine = std::getenv("RELEARN_SERIAL_UPDATE") != nullptr;
  if (!e->has_collective()) {
    e->agreed_serial_env = mine;
    return;
  }
  float h[2] = {mine ? 1.0f : 0.0f, 1.0f};
  {
    DevMem tmp;
    float *d = tmp.alloc<float>(2);
    h2d(e, d, h, sizeof(h));
    rl_allreduce_sum_f32(e, d, 2);
    d2h(e, h, d, sizeof(h));
    ipc_check(e);
  }
  if (h[1] != (float)e->n_ranks)
    throw RlError(RL_ERR_COMM, "the collective's first all-reduce counted " + std::to_string((int)h[1]) + " of " +
                                   std::to_string(e->n_ranks) + " ranks");
  e->agreed_serial_env = h[0] != 0.0f;
}

extern "C" {

int32_t rl_abi_version(void) { return RL_ABI_VERSION; }

int32_t rl_device_count(int32_t *count) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(count, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
  });
}

int32_t rl_engine_create(int32_t device_ordinal, rl_engine **out) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(out, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
      throw RlError(RL_ERR_NO_DEVICE, "no HIP device visible: this engine has no CPU fallback");
    RL_REQUIRE(device_ordinal >= 0 && device_ordinal < n, "device ordinal out of range");
    std::unique_ptr<rl_engine> e(new rl_engine());
    e->device = device_ordinal;
    RL_HIP_CHECK(hipSetDevice(device_ordinal));
    RL_HIP_CHECK(hipGetDeviceProperties(&e->prop, device_ordinal));
    if (std::strncmp(e->prop.gcnArchName, "gfx950", 6) != 0)
      throw RlError(RL_ERR_NO_DEVICE,
                    std::string("device is ") + e->prop.gcnArchName + ", this library is built for gfx950 only");
    RL_HIP_CHECK(hipStreamCreateWithFlags(&e->main_stream, hipStreamNonBlocking));
    RL_HIP_CHECK(hipStreamCreateWithFlags(&e->aux_stream, hipStreamNonBlocking));
    e->stream = e->main_stream;
    RL_HIP_CHECK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    RL_HIP_CHECK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    RL_HIP_CHECK(hipEventCreate(&e->ev_begin));
    RL_HIP_CHECK(hipEventCreate(&e->ev_end));
    e->pinned_bytes = 1 << 16;
    RL_HIP_CHECK(hipHostMalloc(&e->pinned, e->pinned_bytes, hipHostMallocDefault));
    *out = e.release();
  });
}

static void engine_teardown(rl_engine *e);

int32_t rl_engine_destroy(rl_engine *e) {
  if (!e) return RL_OK;
  if (e->live_handles > 0) {
    e->zombie = true;  // torn down when the last child handle goes away
    return RL_OK;
  }
  engine_teardown(e);
  return RL_OK;
}

void engine_release_child(rl_engine *e) {
  e->live_handles -= 1;
  if (e->zombie && e->live_handles <= 0) engine_teardown(e);
}

static void engine_teardown(rl_engine *e) {
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->main_stream);
  (void)hipStreamSynchronize(e->aux_stream);
  if (e->comm_aux && g_rccl.CommDestroy) g_rccl.CommDestroy(e->comm_aux);
  if (e->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(e->comm);
  ipc_teardown(e);
  prof_drain(e);
  for (auto ev : e->prof_event_pool) (void)hipEventDestroy(ev);
  if (e->pinned) (void)hipHostFree(e->pinned);
  (void)hipEventDestroy(e->ev_begin);
  (void)hipEventDestroy(e->ev_end);
  (void)hipEventDestroy(e->ev_fork);
  (void)hipEventDestroy(e->ev_join);
  (void)hipStreamDestroy(e->aux_stream);
  (void)hipStreamDestroy(e->main_stream);
  delete e;
}

int32_t rl_engine_sync(rl_engine *e) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    sync(e);
    // also drain anything a collective library queued on streams of its own
    RL_HIP_CHECK(hipSetDevice(e->device));
    RL_HIP_CHECK(hipDeviceSynchronize());
    ipc_check(e);
  });
}

const char *rl_last_error(const rl_engine *e) { return e ? e->last_error.c_str() : g_last_error_no_engine.c_str(); }

int32_t rl_engine_info(const rl_engine *e, char *name_out, size_t name_cap, char *arch_out, size_t arch_cap,
                       int32_t *compute_units) {
  return guarded(const_cast<rl_engine *>(e), [&] {
    RL_REQUIRE(e, "engine is NULL");
    // (some driver stacks report an empty marketing name: the architecture then stands in for it)
    if (name_out && name_cap) std::snprintf(name_out, name_cap, "%s", e->prop.name[0] ? e->prop.name : e->prop.gcnArchName);
    if (arch_out && arch_cap) std::snprintf(arch_out, arch_cap, "%s", e->prop.gcnArchName);
    if (compute_units) *compute_units = e->prop.multiProcessorCount;
  });
}

int32_t rl_timer_begin(rl_engine *e) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    RL_HIP_CHECK(hipEventRecord(e->ev_begin, e->stream));
  });
}

int32_t rl_timer_end(rl_engine *e, float *elapsed_ms) {
  return guarded(e, [&] {
    RL_REQUIRE(e && elapsed_ms, "NULL argument");
    RL_HIP_CHECK(hipEventRecord(e->ev_end, e->stream));
    RL_HIP_CHECK(hipEventSynchronize(e->ev_end));
    RL_HIP_CHECK(hipEventElapsedTime(elapsed_ms, e->ev_begin, e->ev_end));
  });
}

int32_t rl_engine_set_kernel_variant(rl_engine *e, int32_t variant) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    RL_REQUIRE(variant == 0 || variant == 1, "kernel variant must be 0 (best) or 1 (v1 reference kernels)");
    e->kernel_variant = variant;
  });
}

int32_t rl_engine_set_serial_update(rl_engine *e, int32_t serial) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    e->serial_update = serial != 0;
  });
}

int32_t rl_profile_enable(rl_engine *e, int32_t on) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    sync(e);
    prof_drain(e);
    e->profiling = on != 0;
  });
}

int32_t rl_profile_read(rl_engine *e, double *total_ms_out, uint64_t *launches_out, int32_t reset) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    sync(e);
    prof_drain(e);
    for (int i = 0; i < RL_K_CLASS_COUNT; ++i) {
      if (total_ms_out) total_ms_out[i] = e->prof_ms[i];
      if (launches_out) launches_out[i] = e->prof_launches[i];
      if (reset) {
        e->prof_ms[i] = 0.0;
        e->prof_launches[i] = 0;
      }
    }
  });
}

// ---------------------------------------------------------------- comm
int32_t rl_comm_available(void) {
  return guarded(nullptr, [&] {
    if (std::getenv("RELEARN_LOOPBACK_COMM")) return;
    rccl_load();
  });
}

int32_t rl_comm_library_paths(char *rccl_out, size_t rccl_cap, char *hip_out, size_t hip_cap) {
  return guarded(nullptr, [&] {
    Dl_info info;
    if (rccl_out && rccl_cap) {
      rccl_out[0] = 0;
      if (g_rccl.AllReduce && dladdr((void *)g_rccl.AllReduce, &info) != 0 && info.dli_fname)
        std::snprintf(rccl_out, rccl_cap, "%s", info.dli_fname);
    }
    if (hip_out && hip_cap) {
      hip_out[0] = 0;
      if (dladdr((void *)&hipGetDeviceCount, &info) != 0 && info.dli_fname)
        std::snprintf(hip_out, hip_cap, "%s", info.dli_fname);
    }
  });
}

int32_t rl_comm_unique_id(uint8_t id_out[128]) {
  return guarded(nullptr, [&] {
    RL_REQUIRE(id_out, "id_out is NULL");
    if (std::getenv("RELEARN_LOOPBACK_COMM")) {
      static std::atomic<uint64_t> counter{0};
      std::memset(id_out, 0, 128);
      uint64_t v = ++counter;
      std::memcpy(id_out, &v, sizeof(v));
      return;
    }
    rccl_load();
    rccl_check(g_rccl.GetUniqueId(id_out), "ncclGetUniqueId");
  });
}

int32_t rl_comm_init(rl_engine *e, int32_t rank, int32_t n_ranks, const uint8_t unique_id[128]) {
  return guarded(e, [&] {
    RL_REQUIRE(e && unique_id, "NULL argument");
    RL_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bad rank / n_ranks");
    RL_REQUIRE(!e->has_collective(), "communicator already initialised");
    // rank / n_ranks are set only once the collective exists: a failed initialisation leaves a one-rank engine
    // a single rank needs no communicator; RELEARN_FORCE_RCCL=1 creates a 1-rank one anyway so that the whole
    // RCCL call path (dlopen, ncclCommInitRank, ncclAllReduce on the engine stream) can be exercised on one GPU
    if (std::getenv("RELEARN_LOOPBACK_COMM")) {
      RL_REQUIRE(!e->loopback, "communicator already initialised");
      std::lock_guard<std::mutex> lk(g_loopback_mu);
      std::string key((const char *)unique_id, 128);
      auto &grp = g_loopback_groups[key];
      if (!grp) {
        grp = std::make_shared<LoopbackGroup>();
        grp->n_ranks = n_ranks;
        grp->bufs.assign(n_ranks, nullptr);
        RL_HIP_CHECK(hipSetDevice(e->device));
        RL_HIP_CHECK(hipMalloc((void **)&grp->d_bufs, n_ranks * sizeof(float *)));  // (lives as long as the process)
        if (const char *tw = std::getenv("RELEARN_LOOPBACK_TEST_WEIGHT")) {
          int r = -1;
          float w = 1.0f;
          if (std::sscanf(tw, "%d:%f", &r, &w) == 2 && r >= 0 && r < n_ranks) grp->bad_rank = r, grp->bad_weight = w;
        }
        if (const char *tm = std::getenv("RELEARN_LOOPBACK_TIMEOUT_MS")) {
          long long ms = 0;
          if (std::sscanf(tm, "%lld", &ms) == 1 && ms > 0) grp->deadline = std::chrono::milliseconds(ms);
        }
      }
      RL_REQUIRE(grp->n_ranks == n_ranks, "loopback group: inconsistent n_ranks");
      grp->joined += 1;
      e->loopback = grp.get();
      e->rank = rank;
      e->n_ranks = n_ranks;
      e->agreed_serial_env = std::getenv("RELEARN_SERIAL_UPDATE") != nullptr;  // (one process: one environment)
      return;
    }
    if (n_ranks == 1 && !std::getenv("RELEARN_FORCE_RCCL")) return;
    rccl_load();
    RL_HIP_CHECK(hipSetDevice(e->device));
    UniqueId id;
    std::memcpy(id.bytes, unique_id, 128);
    comm_init_rank_t init = (comm_init_rank_t)(void *)g_rccl.CommInitRank;
    void *comm = nullptr;
    rccl_check(init(&comm, n_ranks, id, rank), "ncclCommInitRank");
    e->comm = comm;
    e->rank = rank;
    e->n_ranks = n_ranks;
    // A second communicator over the same ranks for the auxiliary update chain (rl_actor_critic_update runs the policy
    // and the critic chain on two streams, each with its collectives).  Its unique id is made on rank 0 and handed out
    // through the first communicator — an all-reduce in which only rank 0 contributes (bytes as small integers: exact in
    // f32) — so the caller's bootstrap stays one id.  Whether the job HAS the second communicator is decided
    // collectively: rank 0 joins the hand-out even when it could not make an id (zeros plus a failure flag), a rank with
    // RELEARN_NO_AUX_COMM=1 in its environment vetoes for all, and after the attempt the ranks all-reduce their outcome
    // over the first communicator — one rank without it and every rank drops it (the two chains then run in turn
    // everywhere: ranks that disagreed would issue the critic's collectives on different communicators and hang).
    try {
      const bool want_aux = std::getenv("RELEARN_NO_AUX_COMM") == nullptr;
      UniqueId id2;
      std::memset(id2.bytes, 0, sizeof(id2.bytes));
      bool id_ok = false;
      if (rank == 0 && want_aux) id_ok = g_rccl.GetUniqueId(id2.bytes) == 0;
      float h_id[130];
      for (int i = 0; i < 128; ++i) h_id[i] = rank == 0 && id_ok ? (float)(unsigned char)id2.bytes[i] : 0.0f;
      h_id[128] = rank == 0 && !id_ok ? 1.0f : 0.0f;  // rank 0 has no id to offer
      h_id[129] = want_aux ? 0.0f : 1.0f;             // this rank declines
      DevMem tmp;
      float *d_id = tmp.alloc<float>(130);
      void *comm2 = nullptr;
      try {
        h2d(e, d_id, h_id, sizeof(h_id));
        rccl_check(g_rccl.AllReduce(d_id, d_id, 130, 7, 0, e->comm, e->stream), "ncclAllReduce (second unique id)");
        d2h(e, h_id, d_id, sizeof(h_id));
        const bool attempt = h_id[128] == 0.0f && h_id[129] == 0.0f;
        float outcome = 0.0f;
        if (attempt) {
          for (int i = 0; i < 128; ++i) id2.bytes[i] = (char)(unsigned char)h_id[i];
          if (init(&comm2, n_ranks, id2, rank) == 0 && comm2 != nullptr) outcome = 1.0f;
          else comm2 = nullptr;
        }
        h2d(e, d_id, &outcome, sizeof(outcome));
        rccl_check(g_rccl.AllReduce(d_id, d_id, 1, 7, 0, e->comm, e->stream), "ncclAllReduce (second communicator: outcome)");
        d2h(e, &outcome, d_id, sizeof(outcome));
        if (outcome == (float)n_ranks) {
          e->comm_aux = comm2;
          comm2 = nullptr;
        } else {
          if (rank == 0)
            std::fprintf(stderr, "relearn_hip: no second communicator (%s): update chains will run one after the other "
                                 "on every rank\n",
                         !attempt ? (h_id[129] != 0.0f ? "RELEARN_NO_AUX_COMM on some rank" : "rank 0 could not make an id")
                                  : "ncclCommInitRank failed on some rank");
        }
      } catch (...) {
        if (comm2) g_rccl.CommDestroy(comm2);
        throw;
      }
      if (comm2) g_rccl.CommDestroy(comm2);  // created here, but not everywhere
      comm_agree(e);
    } catch (...) {  // the first communicator could not even carry the agreement: no collective at all
      if (e->comm_aux) g_rccl.CommDestroy(e->comm_aux);
      g_rccl.CommDestroy(e->comm);
      e->comm = e->comm_aux = nullptr;
      e->rank = 0;
      e->n_ranks = 1;
      throw;
    }
  });
}

int32_t rl_comm_init_host(rl_engine *e, int32_t rank, int32_t n_ranks, rl_host_allreduce_fn fn, void *ctx) {
  return guarded(e, [&] {
    RL_REQUIRE(e && fn, "NULL argument");
    RL_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bad rank / n_ranks");
    RL_REQUIRE(!e->has_collective(), "communicator already initialised");
    e->rank = rank;
    e->n_ranks = n_ranks;
    e->host_allreduce = fn;
    e->host_allreduce_ctx = ctx;
    try {
      comm_agree(e);  // (every rank installs its callback at the same point of the job: the first all-reduce runs here)
    } catch (...) {
      e->host_allreduce = nullptr;
      e->host_allreduce_ctx = nullptr;
      e->rank = 0;
      e->n_ranks = 1;
      throw;
    }
  });
}

// Every rank sends pseudo-random payloads that every rank can recompute: small integers, so that the expected sum is
// exact in f32 whatever order a transport adds in.  240 rounds x {2048, 1030, 901, 64, 4} elements: on the mailbox
// transport that is every one of the 32 chunks, both slots many times over, sequence numbers running — a torn or stale
// 64-bit word, or a lost store, shows up as a wrong element.
static inline int32_t selftest_payload(uint32_t round, uint32_t rank, uint32_t i) {
  uint64_t z = ((uint64_t)round << 40) ^ ((uint64_t)rank << 32) ^ (uint64_t)i;
  z += 0x9E3779B97F4A7C15ull;  // splitmix64
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int32_t)(z & 0xFFFF) - 32768;
}

int32_t rl_comm_selftest(rl_engine *e) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    const uint32_t sizes[5] = {2048, 1030, 901, 64, 4};  // IPC_CAP; policy gradient + scalars; critic; one chunk; scalars
    std::vector<float> h(2048);
    DevMem tmp;
    float *d = tmp.alloc<float>(2048);
    for (uint32_t round = 0; round < 240; ++round) {
      const uint32_t count = sizes[round % 5];
      for (uint32_t i = 0; i < count; ++i) h[i] = (float)selftest_payload(round, (uint32_t)e->rank, i);
      h2d(e, d, h.data(), count * sizeof(float));
      rl_allreduce_sum_f32(e, d, count);
      if (round % 16 == 15 || round == 239) {  // (between checks the collectives run back to back, as in an update)
        d2h(e, h.data(), d, count * sizeof(float));
        ipc_check(e);
        for (uint32_t i = 0; i < count; ++i) {
          int32_t want = 0;
          for (int r = 0; r < e->n_ranks; ++r) want += selftest_payload(round, (uint32_t)r, i);
          if (h[i] != (float)want)
            throw RlError(RL_ERR_COMM, "collective self-test: wrong sum at element " + std::to_string(i) + " of round " +
                                           std::to_string(round));
        }
      }
    }
  });
}

int32_t rl_comm_destroy(rl_engine *e) {
  return guarded(e, [&] {
    RL_REQUIRE(e, "engine is NULL");
    e->host_allreduce = nullptr;
    e->host_allreduce_ctx = nullptr;
    if (e->comm_aux) {
      RL_HIP_CHECK(hipStreamSynchronize(e->aux_stream));
      rccl_check(g_rccl.CommDestroy(e->comm_aux), "ncclCommDestroy");
      e->comm_aux = nullptr;
    }
    if (e->comm) {
      sync(e);
      rccl_check(g_rccl.CommDestroy(e->comm), "ncclCommDestroy");
      e->comm = nullptr;
    }
    e->loopback = nullptr;  // groups live for the life of the process (test facility)
    if (e->ipc_box) {
      sync(e);
      ipc_teardown(e);
    }
    e->ipc_active = false;
    e->rank = 0;
    e->n_ranks = 1;
  });
}

// live device memory of the whole process — every allocation a handle's DevMem has made and not yet freed (test hook:
// what is created is released, on every path)
int32_t rl_debug_device_memory(uint64_t *live_bytes, uint64_t *live_allocations) {
  if (live_bytes) *live_bytes = g_device_bytes.load();
  if (live_allocations) *live_allocations = g_device_allocations.load();
  return RL_OK;
}

}  // extern "C"
