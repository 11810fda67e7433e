// mbd_internal.h — what the translation units of libmbd_hip.so's host side share (NOT part of the boundary: the C ABI is
// include/mbd_hip.h): the owners of runtime resources, the env handle, error reporting, the test levers, what plans and
// sweeps do alike — every record, once: the struct, its check_*, set and peek (the adapt record too, which only plans hold); the
// launches of a record whose single and batch kernels are step kernels (elites, to-go) are free functions of each handle unit over
// the shared struct — and the functions one unit defines for the others.
// Units: mbd_env.hip (library, levers, envs, the rollout launch), mbd_records.hip (every record's members, the check_* family and
// the refusals plans and sweeps share, the mbd_debug_* entries that launch record kernels or none), mbd_plan.hip (plans: one
// reverse-diffusion step and the loops over it), mbd_sweep.hip (sweeps: several plans per launch), mbd_exchange.hip (the
// in-library exchange), mbd_debug_math.hip (mbd_math.h over arrays); mbd_pk2.hip, mbd_planar.hip and mbd_hot3d.hip hold rollout
// instantiations only.  mbd_ring.h: the ring logs' arithmetic, which includes nothing and is tested on the host alone.
// No kernel is visible from here: a static kernel is emitted by every unit that sees it, so a unit that launches kernels includes
// their header itself (mbd_env.hip: mbd_env_kernels.h; mbd_records.hip: mbd_record_kernels.h; mbd_plan.hip, mbd_sweep.hip:
// mbd_step_kernels.h).  This header takes the argument structs its records keep by value from mbd_step_args.h, and the constants
// and host-and-device functions the kernel headers and the host code share from mbd_step_device.h, which defines no kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mbd_hip.h"
#include "mbd_kernels.h"
#include "mbd_launch.h"
#include "mbd_ring.h"
#include "mbd_step_args.h"
#include "mbd_step_device.h"

using namespace mbd;

// a function or member that crosses units but not the library's boundary: it stays out of the library's symbol list
#define MBD_HIDDEN __attribute__((visibility("hidden")))

// error reporting (mbd_env.hip): sets the thread-local message of mbd_last_error() and returns `code`
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(MBD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
// the same for a function of this library that has already set the message
#define MBD_TRY(expr)                \
  do {                               \
    int _rc = (expr);                \
    if (_rc != MBD_OK) return _rc;   \
  } while (0)


inline int device_count_quiet() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

// ---- host PRNG (jax.random.split) --------------------------------------------------------------------
inline void host_split(const uint32_t key[2], int num, int impl, uint32_t* keys) {
  if (impl == MBD_PRNG_PARTITIONABLE) {
    for (int j = 0; j < num; ++j) threefry2x32(key[0], key[1], 0u, (uint32_t)j, keys[2 * j], keys[2 * j + 1]);
    return;
  }
  for (int e = 0; e < 2 * num; ++e) keys[e] = random_bits32(key[0], key[1], 0, (uint64_t)e, (uint64_t)(2 * num));
}

enum EnvKind { ENV_CAR2D = 0, ENV_MODEL = 1 };
constexpr int kLdsN = 36 * 1024;  // candidates whose logp0 fits the score kernel's LDS (144 KB of the CU's 160)


// ---- owners of runtime resources ---------------------------------------------------------------------------------------
// What a handle struct holds of the device, by type: each owner releases in its destructor, so a handle's destructor lists
// nothing, and an exit of a create function, early or not, leaks nothing.  Move-only.  Allocation and creation are calls
// that return hipError_t (HIP_TRY at the call site), not constructors: what is created on first use stays that way.
// Members are destroyed in reverse order of declaration: a handle declares its streams in front of its buffers.
template <typename T>
class DevBuf {  // n elements of device memory; converts to T*, so kernel argument lists read as with a raw pointer
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
  ~DevBuf() { (void)hipFree(p_); }
  // n elements, whatever it held before.  The one spelling of free, null, allocate, record: a failed allocation leaves an
  // empty buffer.  fine_grained: hipDeviceMallocFinegrained memory (the exchange's window)
  hipError_t alloc(size_t n, bool fine_grained = false) {
    hipError_t e = hipFree(p_);
    p_ = nullptr; n_ = 0;
    if (e != hipSuccess) return e;
    e = fine_grained ? hipExtMallocWithFlags((void**)&p_, sizeof(T) * n, hipDeviceMallocFinegrained) : hipMalloc(&p_, sizeof(T) * n);
    if (e != hipSuccess) p_ = nullptr;
    else n_ = n;
    return e;
  }
  hipError_t grow(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }  // at least n elements; the contents do not survive
  // The three moves of an entry that runs a kernel on host arrays (the mbd_debug_* entries, the peeks).  None synchronises: that
  // stays with the caller.  (Inlined, so that the library's symbol list does not grow.)  upload: n elements holding host[0 .. n)
  __forceinline__ hipError_t upload(const T* host, size_t n) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemcpy(p_, host, sizeof(T) * n, hipMemcpyHostToDevice);
  }
  // n elements with every bit set: what a kernel leaves unwritten reads back as NaN, or -1
  __forceinline__ hipError_t alloc_poisoned(size_t n) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemset(p_, 0xff, sizeof(T) * n);
  }
  // the first n elements into host[0 .. n); nothing for a NULL host (an output the caller did not ask for) or n == 0
  __forceinline__ hipError_t download(T* host, size_t n) const {
    return host && n ? hipMemcpy(host, p_, sizeof(T) * n, hipMemcpyDeviceToHost) : hipSuccess;
  }
  operator T*() const { return p_; }
  T* get() const { return p_; }  // (where no conversion happens by itself: a deduced parameter, an operand of ?:)

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

class Stream {  // a non-blocking stream
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { std::swap(s_, o.s_); return *this; }
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  hipError_t create() { return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e_, flags); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

class PinnedWord {  // one int of pinned host memory the device stores into (a progress word), zero at creation
 public:
  PinnedWord() = default;
  PinnedWord(PinnedWord&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  PinnedWord& operator=(PinnedWord&& o) noexcept { std::swap(h_, o.h_); return *this; }
  ~PinnedWord() { if (h_) (void)hipHostFree(h_); }
  hipError_t create() {
    const hipError_t e = hipHostMalloc((void**)&h_, sizeof(int), hipHostMallocDefault);
    if (e == hipSuccess) *h_ = 0;
    return e;
  }
  operator int*() const { return h_; }

 private:
  int* h_ = nullptr;
};

class PinnedBuf {  // n floats of pinned host memory mapped into the device's address space (a session's staging and mailbox)
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : h_(o.h_), d_(o.d_) { o.h_ = nullptr; o.d_ = nullptr; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(h_, o.h_); std::swap(d_, o.d_); return *this; }
  ~PinnedBuf() { release(); }
  void release() {
    if (h_) (void)hipHostFree(h_);
    h_ = nullptr; d_ = nullptr;
  }
  hipError_t alloc(size_t n) {  // zeroed; whatever it held before is gone
    release();
    hipError_t e = hipHostMalloc((void**)&h_, sizeof(float) * n, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) { h_ = nullptr; return e; }
    memset(h_, 0, sizeof(float) * n);
    e = hipHostGetDevicePointer((void**)&d_, h_, 0);
    if (e != hipSuccess) release();
    return e;
  }
  float* host() const { return h_; }
  float* dev() const { return d_; }  // the same bytes as the device addresses them

 private:
  float* h_ = nullptr;
  float* d_ = nullptr;
};

// ---- the device ring logs (mbd_ring.h has the arithmetic) -------------------------------------------------------------
// A record's log of its ticks or steps on the device: entry j at j % cap, `count` entries ever written (host bookkeeping: the
// kernels are handed the slot).  kLogCap: the most a log holds per plan.  ring_slot: where the next entry goes, count advanced.
// ring_read: the most recent min(n, count, cap) entries of ONE ring — d_ring [cap][width], a plan's own (the caller adds plan
// k's cap width elements) — into host out, oldest first, by at most two copies; nothing for a NULL out.
constexpr int kLogCap = 65536;
static inline long long ring_slot(long long& count, long long cap) { return count++ % cap; }
template <typename T>
static int ring_read(const T* d_ring, int width, long long count, long long cap, long long n, T* out) {
  const RingRuns r = ring_recent(count, cap, n);
  for (int i = 0; out && i < 2; ++i) {
    if (r.len[i]) HIP_TRY(hipMemcpy(out, d_ring + r.first[i] * width, sizeof(T) * r.len[i] * width, hipMemcpyDeviceToHost));
    out += r.len[i] * width;
  }
  return MBD_OK;
}

struct mbd_env : EnvShape {  // (the shape: derive_shape, at creation; car2d keeps the defaults)
  int kind = ENV_MODEL;
  int device = 0;
  std::string name;
  mbd_model_t model;
  DevBuf<mbd_model_t> d_model;
  DevBuf<float> d_xref;
  bool has_xref = false;
  float rew_xref = 0.0f;
  int n_cus = 256;  // compute units of the device (hipDeviceProp_t::multiProcessorCount; four SIMDs each)
  DevBuf<signed char> d_lane_tab;
  DevBuf<LaneRec3> d_lane_rec;  // [3][16]: per-lane constants of the 3-D kernels (lane = link; the DPP layout; the
                                // DPP layout with helper lanes)
  unsigned long long* dbg_clock = nullptr;  // per env, caller-owned device buffer (mbd_debug_set_clock_buffer; probes only)
  // scratch for the single-env step path
  DevBuf<float> d_s_in, d_act, d_s_out, d_rew;
  ~mbd_env() { (void)hipSetDevice(device); }  // (the buffers release themselves, on the env's device)
  int state_size() const { return kind == ENV_CAR2D ? 3 : model.n_links * MBD_LINK_STATE; }
  int action_size() const { return kind == ENV_CAR2D ? 2 : model.n_act; }
  int observation_size() const;
};

// Lazy candidates of a plan's rollout (RolloutParams): d_us holds normals, actions are formed at the fetch; and the
// optional noise job for the NEXT step, which rides in spare workgroups of the launch when the rollout leaves CUs idle.
struct LazyArgs {
  const float* ybar = nullptr;  // Ybar_i [H][Nu]
  float sigma = 0.0f;
  float* nz_out = nullptr;      // [nz_N][nz_HNu] normals of the next step, or nullptr: no job
  const float* nz_g = nullptr;  // the noise shape [nz_HNu] that step samples under (device), or nullptr: none
  // the noise basis [H][nz_knots] that step samples under (device), or nullptr: none.  A job under a basis is knot_noise_kernel's,
  // never the launch's: launch_rollout leaves it alone (nz_fused stays false) and the caller runs it on its second stream
  const float* nz_W = nullptr;
  int nz_knots = 0;
  uint32_t nz_key[2] = {0, 0};
  int nz_impl = 0, nz_N = 0, nz_HNu = 0;
  bool nz_fused = false;        // out: the job went into this launch (false: the caller runs it elsewhere)
  int* progress = nullptr;      // RolloutParams.progress / progress_val
  int progress_val = 0;
};
// What the normals of a diffusion step are made under: the noise shape g [HNu] (mbd_noise_shape) and the noise basis
// W [H][knots] (mbd_noise_basis), both device tables of the plan or sweep, nullptr: none.  The tag of a prepared buffer.
struct NoiseSpec {
  const float* g = nullptr;
  const float* W = nullptr;
  int knots = 0;
  bool operator==(const NoiseSpec& o) const { return g == o.g && W == o.W && knots == o.knots; }
};
// the host's view of a progress word (pinned host memory the device stores into)
static inline int progress_read(const int* h) { return __atomic_load_n(h, __ATOMIC_ACQUIRE); }
static inline void progress_reset(int* h) { __atomic_store_n(h, 0, __ATOMIC_RELEASE); }  // (between loops, the streams idle)
// how long a host loop that keeps step with the device through the progress word waits before it falls back to ordering
// the streams with an event (steady_clock also counts system pauses)
constexpr int kInStepWaitMs = 20;
// Waits until the progress word has reached `target`, looking every sleep_us, for limit_ms at the most; whether it has (the
// last look comes after the limit).  A stream that is legitimately slow (a shared or time-sliced GPU, a profiler, a system
// pause) is not an error: the caller then orders its streams with an event instead.
inline bool progress_wait(const int* h, int target, int limit_ms, int sleep_us) {
  const auto w0 = std::chrono::steady_clock::now();
  while (progress_read(h) < target && std::chrono::steady_clock::now() - w0 < std::chrono::milliseconds(limit_ms))
    std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
  return progress_read(h) >= target;
}
// workgroups (of 256) of a launch that generates `normals` normals grid-stride: a thread makes one, or two of an unpartitioned
// stream; cap: 65536 for a plan, 4096 per plan of a sweep
inline unsigned noise_blocks(int prng_impl, uint64_t normals, uint64_t cap) {
  const uint64_t items = prng_impl == MBD_PRNG_PARTITIONABLE ? normals : (normals + 1) / 2;
  const uint64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks < cap ? blocks : cap);
}
// The pool of event pairs that time the rollout launches of a plan or a sweep (mbd_*_kernel_time): begin in front of the
// launch, end behind it, both nothing while the pool is off; pairs are created as they are needed and reused after a reset.
struct TimingPool {
  bool on = false;
  std::vector<std::pair<Event, Event>> pairs;
  size_t used = 0;
  int begin(hipStream_t s) {
    if (!on) return MBD_OK;
    if (used == pairs.size()) {
      Event a, b;
      HIP_TRY(a.create(hipEventDefault));
      HIP_TRY(b.create(hipEventDefault));
      pairs.emplace_back(std::move(a), std::move(b));
    }
    HIP_TRY(hipEventRecord(pairs[used++].first, s));
    return MBD_OK;
  }
  int end(hipStream_t s) {
    if (on) HIP_TRY(hipEventRecord(pairs[used - 1].second, s));
    return MBD_OK;
  }
  // the mean over the pairs used since the last reset, once the device is idle
  int average(float* avg_ms_out, int* count_out, bool reset) {
    HIP_TRY(hipDeviceSynchronize());
    double tot = 0.0;
    for (size_t k = 0; k < used; ++k) {
      float ms = 0.0f;
      HIP_TRY(hipEventElapsedTime(&ms, pairs[k].first, pairs[k].second));
      tot += ms;
    }
    if (avg_ms_out) *avg_ms_out = used ? (float)(tot / (double)used) : 0.0f;
    if (count_out) *count_out = (int)used;
    if (reset) used = 0;
    return MBD_OK;
  }
};
// ---- defined in mbd_env.hip ------------------------------------------------------------------------------------------
// test / A-B levers (one process-wide table, include/mbd_hip_debug.h): -1 = not set
int lever(const char* name);
bool env_flag(const char* name);
// the device-free facts of a model the launch paths need (env creation; mbd_debug_rollout_choice): MBD_OK, or the error
// of a model no instantiation is built for
int derive_shape(const mbd_model_t& m, EnvShape& s);
// Everything about a rollout launch of B candidates, decided in one place (mbd_env.hip::choose_rollout).
struct RolloutChoice {
  RolloutKernel kernel = nullptr;  // host stub of the instantiation; nullptr: none serves the model
  dim3 grid, block;                // the rollout's own workgroups (launch_rollout adds the noise job's and the XCD pin's)
  size_t lds = 0;                  // dynamic LDS each workgroup reserves
  int cpw = 0;                     // RolloutParams::cpw: candidates per wavefront of an early-out launch, 0: filled
  int spw = 1;                     // candidates a wavefront of the launch holds (cpw, or the layout's, twice that two per lane)
  int wpe = 1;                     // two-candidates-per-lane launches: wavefronts per SIMD the instantiation is asked for
  bool xcd_pin = false;            // the launch goes to one XCD (RolloutParams::xcd_pin)
  bool fuses_noise = false;        // a launch with a noise job takes it into spare workgroups
  bool fuses_logpd = false;        // the instantiation accumulates the demo log-density itself (RolloutParams::lp)
  std::string name() const;        // the instantiation's symbol, demangled (what profilers show)
};
// sweep = {plan_N, plan_state_stride, plan_ybar_stride} (RolloutParams), or nullptr: one plan; has_xref: the env has a demo
RolloutChoice choose_rollout(const EnvShape& s, const mbd_model_t& m, int n_cus, int B, int H, const int* sweep, bool has_xref);
// choose_rollout for an env (car2d: no choice — its rollout is not a RolloutParams instantiation)
RolloutChoice rollout_choice(const mbd_env* env, int B, int H, const int* sweep = nullptr);
// Whether a launch of that choice takes a noise job of nz_N x nz_HNu normals into its own workgroups (launch_rollout's
// decision, for the plans that ask in advance): fuses_noise, and for a launch pinned to one XCD enough noise workgroups —
// a sharded plan generates the normals of ALL N candidates beside a rollout of its shard only.  false: the job runs on the
// plan's second stream, which then has to be ordered behind the buffer's last reader.
bool rollout_takes_noise(const RolloutChoice& c, int nz_impl, int nz_N, int nz_HNu);
// An ensemble launch (RolloutParams::ens_M): the candidates d_us [N] on each of the M member envs, outputs [M][N]...; the
// launch's switches, tables and choice are env's (mbd_plan_set_ensemble has checked that the members share them).
struct EnsArgs {
  int M = 0;
  mbd_env* const* members = nullptr;  // [M], none NULL
};
// the choice of an ensemble's rollout over M N candidates, and whether ONE launch serves it (N a multiple of the candidates
// per wavefront of that choice); otherwise launch_rollout runs M launches of N candidates, one per member.  members [M],
// none NULL: the choice compiles in only what holds for every one of them (EnvShape::unit_ib)
RolloutChoice ensemble_choice(const mbd_env* env, int M, mbd_env* const* members, int N, int H, bool* one_launch);
// launch of the env's rollout instantiation; sweep as above.  ens: B is the plan's N, the outputs hold M rows of it.  d_lp: the demo log-densities [B] accumulated inside the
// rollout (RolloutParams::lp) — only where the choice's fuses_logpd says so (the caller then passes d_lp instead of d_xpos
// and skips launch_logpd).  d_xref: the demo table the launch reads in place of the env's (RolloutParams::xref; a tick's window
// of an episode with a demo record, [n_track][kXrefRows][3]), nullptr: the env's own
int launch_rollout(mbd_env* env, const float* d_state0, const float* d_us, int B, int H, float* d_rewss, float* d_rews,
                   float* d_xpos, float* d_state_final, hipStream_t stream, LazyArgs* lz = nullptr, const int* sweep = nullptr,
                   float* d_lp = nullptr, const EnsArgs* ens = nullptr, const float* d_xref = nullptr);
// whether the device is a whole 8-XCD part (the premise of the XCD-pinned launch forms)
bool device_has_eight_xcds(const mbd_env* env);
int launch_logpd(const mbd_env* e, const float* d_xpos, int B, int H, float* d_out, hipStream_t s, const float* d_xref = nullptr);
// ---- defined in mbd_records.hip (plant_tick_draw, at the end: mbd_plan.hip) ------------------------------------------
// noise schedule (mbd_planner.py:84-87)
void host_schedule(float beta0, float betaT, int Nd, std::vector<float>& alphas, std::vector<float>& alphas_bar,
                   std::vector<float>& sigmas);
// the refusals of a plant record (include/mbd_hip.h mbd_mpc_plant) against the env that plans — host arithmetic, no launch
int check_mpc_plant(const mbd_env* env, const mbd_mpc_plant* rec);
// the refusals of an episode's configuration that plans and sweeps share (include/mbd_hip.h mbd_mpc_config), in their order
// (has_demo_rec: the handle carries a demo record — a demo plan without one has no clock for its demo and stays refused;
// has_sigma_rec: it carries a sigma record — a path-integral handle without one stays refused; pi_sessions: the call opens a
// sweep's session, which path-integral sweeps do not have, record or not)
int check_mpc_config(const mbd_plan_config& c, const mbd_mpc_config* mc, bool has_demo_rec, bool has_sigma_rec,
                     bool pi_sessions = false);
// The sigma record of a path-integral plan or sweep (include/mbd_hip.h mbd_mpc_sigma) as the handle keeps it, with what the two
// handles do alike: the refusals the record alone decides against the handle's update_method, in the header's order, each naming
// the field (check_mpc_sigma: host arithmetic, before any device access), and the set call behind its NULL-handle, update_method
// and session checks (nullptr clears).  d_log: the sigmas of the last episode, episode-major [P][T + 1][2] — what tick t started
// from and ended with; the boundary behind the last tick writes slot T's first float —, ticks / episodes: its T and P, 0: none
// yet (mbd_*_peek_mpc_sigma).
struct SigmaRec {
  bool has = false;
  float cold = 1.0f, warm = 1.0f, gain = 0.0f;
  int ticks = 0, episodes = 0;
  int log_ticks = 0;  // the T the log was laid out for (start)
  DevBuf<float> d_log;
  int set(const mbd_mpc_sigma* rec, int update_method);
  // in front of an episode of T ticks and P episodes: room for the log (a session: T = 1)
  int start(int T, int P);
  long long stride() const { return 2ll * (log_ticks + 1); }
  // the launch in front of a cold tick (cold: the carried sigmas [P] and slot t's first float take sigma_cold) or at the
  // boundary behind tick t (slot t's second float takes the carried sigma, which becomes the next tick's; slot t + 1's first)
  void launch(float* d_sigma, int P, int t, bool cold_tick, hipStream_t s) const;
  // HOST sigmas_out [T][2] of episode k of the last run
  int peek(int device, int k, float* sigmas_out, const char* what) const;
};
int check_mpc_sigma(const mbd_mpc_sigma* rec, int update_method);
// the refusals of a noise-shape record (include/mbd_hip.h mbd_noise_shape) against a handle's Hsample x action_size, in the
// header's order, each naming the field — host arithmetic on the record's own table, before any device access
int check_noise_shape(const mbd_noise_shape* rec, int Hsample, int action_size);
// the refusals of a noise-basis record (include/mbd_hip.h mbd_noise_basis) of a handle with Hsample rows, likewise
int check_noise_basis(const mbd_noise_basis* rec, int Hsample);
// The noise shape and the noise basis of a plan or a sweep (mbd_*_set_noise_shape, mbd_*_set_noise_basis) as the handle keeps them:
// the tables g [HNu] and W [Hsample][knots] on the device and when each is in force; d_knot_z: the scratch z knot_noise_kernel fills
// in front of shift_kernel where candidates are materialised (the caller says how many elements).  The samplers take the tables as
// pointers, nullptr for a flat step.  shape_always: every step outside the warm ticks of an episode (the phase calls, a run, tick 0);
// shape_warm: the steps of the ticks t >= 1, where either mode is in force; spec: with the basis beside it, each under its own
// `when` — the caller's tables only (a plan's adapt record stands its own table in: mbd_plan.hip noise_spec).  set_shape, set_basis:
// behind the handle's NULL and session checks and check_noise_*, (nullptr clears) — they wait for the device, since a step in flight,
// or normals being prepared ahead, may still read the previous table.
struct NoiseRec {
  bool has_shape = false, has_basis = false;
  int shape_when = MBD_NOISE_ALWAYS, basis_when = MBD_NOISE_ALWAYS, knots = 0;
  DevBuf<float> d_shape, d_basis, d_knot_z;
  const float* shape_always() const { return has_shape && shape_when == MBD_NOISE_ALWAYS ? d_shape.get() : nullptr; }
  const float* shape_warm() const { return has_shape ? d_shape.get() : nullptr; }
  NoiseSpec spec(bool warm_tick) const {
    NoiseSpec ns;
    ns.g = warm_tick ? shape_warm() : shape_always();
    if (has_basis && (warm_tick || basis_when == MBD_NOISE_ALWAYS)) {
      ns.W = d_basis.get();
      ns.knots = knots;
    }
    return ns;
  }
  MBD_HIDDEN int set_shape(const mbd_noise_shape* rec, int HNu, int device);
  MBD_HIDDEN int set_basis(const mbd_noise_basis* rec, int Hsample, size_t knot_z_elems, int device);
};
// The delay record of a plan or a sweep (include/mbd_hip.h mbd_mpc_delay) as the handle keeps it — rows0 copied to the host, it
// goes to the device when an episode starts — with what the two handles do alike: the refusals the record alone decides, in the
// header's order, each naming the field (check_mpc_delay: host arithmetic, before any device access), the set call behind
// its NULL-handle check (nullptr clears), and the run call's refusal against its exec_steps.  pred_ticks: T of the last episode
// run with the record, 0: none yet (mbd_*_peek_mpc_predicted).
struct DelayRec {
  bool has = false;
  int D = 0, n_rows = 0, pred_ticks = 0;
  std::vector<float> rows0;  // [n_rows][action_size]
  int set(const mbd_mpc_delay* rec, int action_size);
  int check_run(int exec_steps) const;
  // the committed queue of `copies` episodes at the start of an episode, [copies][D E Nu] on the device (rows0, or zeros)
  int upload(float* d_queue, int copies, int E, int Nu, hipStream_t s) const;
};
int check_mpc_delay(const mbd_mpc_delay* rec, int action_size);
// The demo record of a plan or a sweep (include/mbd_hip.h mbd_mpc_demo) as the handle keeps it, with what the two handles do
// alike.  set: the refusals in the header's order, each naming the field — host arithmetic, before any device access — then the
// clip's copy onto the env's device (nullptr clears).  K, C: the clip's tracks and floats per row (n_track and 3; car2d 1 and 2).
// An episode grows the buffers (start), fills the window table in one launch (start), hands tick t its window (window) and the
// executed rows' rollout its slice of the position log, and ends with the error launch (finish).  ticks / exec / episodes: T, E
// and P of the last episode run with the record, 0: none yet (mbd_*_peek_mpc_track).
struct DemoRec {
  bool has = false;
  int L = 0, c0 = 0, K = 1, C = 3;
  float rew_xref = 0.0f;
  int ticks = 0, exec = 0, episodes = 0;
  DevBuf<float> d_clip, d_windows, d_xlog, d_err;
  int set(const mbd_env* env, const mbd_plan_config& cfg, const mbd_mpc_demo* rec);
  // the plant env of an episode with the record: the positions it writes must be the tracked links' of the plan's env
  int check_plant(const mbd_env* env, const mbd_env* plant) const;
  int start(int T, int P, int E, int D, hipStream_t s);
  const float* window(int t) const { return d_windows + (size_t)t * K * kXrefRows * C; }
  float* xlog(int t, int P, int E, int k = 0) const { return d_xlog + ((size_t)t * P + k) * E * K * 3; }
  int finish(int T, int P, int E, hipStream_t s);
  // a session (mbd_plan_mpc_open) has no table: session_start forgets the last episode's logs and makes room for ONE window,
  // session_window fills it with tick t's — the window start()'s table holds at slot t — by one launch of the same kernel
  int session_start();
  int session_window(long long t, int E, int D, hipStream_t s);
  // HOST err_out [T E][K] and windows_out [T][K][kXrefRows][C] of episode k of the last run; either may be NULL
  int peek(int device, int k, float* err_out, float* windows_out, const char* what) const;
};
// The objective record of a plan or a sweep (include/mbd_hip.h mbd_objective) as the handle keeps it, with what the two handles do
// alike.  check_objective: the refusals the record alone decides against the handle's Hsample x action_size, in the header's
// order, each naming the field — host arithmetic on the record's own tables, before any device access —, and the f32
// left-to-right sum of row_weight (*wsum_out; untouched when row_weight is NULL).  set: behind the handle's NULL and session checks
// and check_objective, whose sum it is handed (nullptr clears); copies the tables onto the device for P plans of N candidates (a plan: P = 1; max_rows: the most rows a step's
// launch scores — M N under an ensemble record).  prev: the previous action every plan's steps take their rate cost against,
// [P][Nu] on the device or nullptr: none — d_prev0 (clip(prev0), or nullptr) outside episodes; an episode or a session points it
// at d_prev, which episode_start fills where the first tick has a previous action and tick_advance re-forms per tick, and
// episode_end puts it back.
struct ObjectiveRec {
  bool has = false, has_w = false, has_prev0 = false, stepped = false;
  float effort = 0.0f, rate = 0.0f, wsum = 0.0f;
  int P = 1, N = 0, H = 0, Nu = 0, rows = 0;  // rows: of the last step's launch, per plan
  DevBuf<float> d_w, d_q, d_prev0, d_prev, d_ret, d_cost;
  const float* prev = nullptr;
  int set(const mbd_objective* rec, float wsum_, int device, int P_, int N_, int H_, int Nu_, size_t max_rows);
  bool costs() const { return effort != 0.0f || rate != 0.0f; }
  // the launch between a rollout and its score: a plan's (ybar_stride < 0: objective_kernel) or a sweep's P plans.  d_rewss
  // [B][H] and d_rews [B] are the rollout's outputs, d_rews is rewritten in place; B, row0: ObjectiveArgs
  int launch(const float* d_rewss, float* d_rews, int B, int row0, const float* d_cand, bool lazy, float sigma,
             const float* d_ybar, long long ybar_stride, hipStream_t s);
  // the same launch over B materialised plans [P][B][H][Nu] that are not a step's candidates (a pick record's slots): row b is plan
  // b of d_plans, results into the caller's d_ret_keep / d_cost_keep [P][B]; what mbd_*_peek_objective shows stays the last step's
  int launch_rows(const float* d_rewss, float* d_rews, int B, const float* d_plans, float* d_ret_keep, float* d_cost_keep, bool batch,
                  hipStream_t s);
  // in front of an episode's or a session's first tick: d_queue_last — row D E - 1 of episode 0's committed queue [P][Q] on the
  // device, or nullptr: no delay record
  int episode_start(const float* d_queue_last, long long Q, hipStream_t s);
  // behind a tick's last update kernel, in front of its boundary kernel: d_row — row E-1 of episode 0's M_t, episode k's
  // stride floats further
  int tick_advance(const float* d_row, long long stride, hipStream_t s);
  void episode_end() { prev = has_prev0 ? d_prev0.get() : nullptr; }
  // HOST ret_out [rows], cost_out [min(rows, N)] of plan k's last step (env: the handle's, looked at behind the state checks)
  int peek(const mbd_env* env, int k, float* ret_out, float* cost_out, const char* what) const;
};
int check_objective(const mbd_objective* rec, int Hsample, int action_size, float* wsum_out);
// The value record of a plan or a sweep (include/mbd_hip.h mbd_value) as the handle keeps it, with what the two handles do alike.
// check_value: the refusals the record alone decides against the env's state_size and kind, in the header's order, each naming the
// field — host arithmetic on the record's own tables, before any device access.  set: behind the handle's NULL, session and ensemble
// checks and check_value (nullptr clears); copies the net onto the device, every layer transposed, and makes room for the final
// states and the V of max_rows rows (a plan: its shard; a sweep: P N) and of the 3 P slots of a pick record.  final(): what a
// rollout launch is handed as d_state_final — nullptr without a record, so that a launch without one is what it was.  launch: the
// kernel over B rows of d_fin, d_rews rewritten in place, V into d_v_keep;
// launch_step: the same over the step's own buffers, what peek shows.
struct ValueRec {
  bool has = false, stepped = false;
  int S = 0, n_layers = 0, act = 0, rel = 0, rows = 0;
  size_t max_rows = 0;
  int width[4] = {0, 0, 0, 0};
  float scale = 0.0f;
  DevBuf<float> d_net;  // center [S] | in_scale [S] | per layer: Wt [K][width] | b [width]
  size_t off_W[4] = {0, 0, 0, 0}, off_b[4] = {0, 0, 0, 0};
  DevBuf<float> d_final, d_v, d_pick_final, d_pick_v, d_eval_in, d_eval_v;
  int set(const mbd_value* rec, const mbd_env* env, size_t max_rows_, int P);
  float* final() const { return has ? d_final.get() : nullptr; }
  float* pick_final() const { return has ? d_pick_final.get() : nullptr; }
  int launch(const float* d_fin, float* d_rews, int B, float* d_v_keep, hipStream_t s) const;
  int launch_step(float* d_rews, int B, hipStream_t s) {
    if (!has) return MBD_OK;
    rows = B;
    stepped = true;
    return launch(d_final, d_rews, B, d_v, s);
  }
  int peek(const mbd_env* env, float* v_out, const char* what) const;
  int eval(const mbd_env* env, const float* states, int B, float* v_out, const char* what);
};
int check_value(const mbd_value* rec, int state_size, bool rigid_body);
// The zone record of a plan or a sweep (include/mbd_hip.h mbd_zones) as the handle keeps it, with what the two handles do alike.
// check_zones: the refusals the record alone decides against the env's n_track, in the header's order, each naming the field — host
// arithmetic, before any device access.  set: behind the handle's NULL, session, env, demo, shard and record checks and check_zones
// (nullptr clears); makes room for the positions, pen and clr of max_rows rows of H steps and K tracks.  update: the table alone —
// host state, since the table travels as kernel arguments.  xpos(): what a planning rollout is handed as d_xpos — nullptr without
// a record, so that a launch without one is what it was.  launch: the kernel over B rows of d_x; launch_step: the same over the
// step's own buffers, what peek shows.  An episode logs its executed steps: start makes
// room for the positions [T P E][K][3] and the log [T P E] twice, log runs the kernel over one tick's executed rows of all P episodes.
struct ZoneRec {
  bool has = false, stepped = false;
  mbd_zones tab{};
  int K = 0, H = 0, rows = 0;
  int ticks = 0, exec = 0, episodes = 0;
  DevBuf<float> d_x, d_pen, d_clr, d_xlog, d_log_pen, d_log_clr;
  int set(const mbd_zones* rec, const mbd_env* env, size_t max_rows, int H_);
  int update(const mbd_zones* rec, const mbd_env* env, const char* what);
  float* xpos() const { return has ? d_x.get() : nullptr; }
  int launch(const float* d_xp, float* d_rews, int B, int H_, float* d_pen_keep, float* d_clr_keep, float* d_step_pen,
             float* d_step_clr, hipStream_t s) const;
  int launch_step(float* d_rews, int B, hipStream_t s) {
    if (!has) return MBD_OK;
    rows = B;
    stepped = true;
    return launch(d_x, d_rews, B, H, d_pen, d_clr, nullptr, nullptr, s);
  }
  // the plant env of an episode with the record: the positions it writes must be the tracked links' of the planning env
  int check_plant(const mbd_env* env, const mbd_env* plant) const;
  int start(int T, int P, int E);
  float* xlog(int t, int P, int E, int k = 0) const { return has ? d_xlog.get() + ((size_t)t * P + k) * E * K * 3 : nullptr; }
  // behind the rollout of tick t's executed rows: s_t and clr_t of the P E steps into the log, ONE launch
  int log(int t, int P, int E, hipStream_t s) const;
  int peek(const mbd_env* env, int k, int N, float* pen_out, float* clr_out, const char* what) const;
  // HOST pen_out, clr_out [T E] of episode k of the last run
  int peek_mpc(const mbd_env* env, int k, float* pen_out, float* clr_out, const char* what) const;
};
int check_zones(const mbd_zones* rec, int n_track);
// the refusals of a zone record the handle's env and config decide, behind check_zones (handle: "plan" / "sweep"); and the refusal of
// a record beside a zone record (who: how the refused record's messages begin)
int check_zones_handle(const mbd_env* env, const mbd_plan_config& c, const char* handle);
int refuse_beside_zones(const char* who, const char* handle = "plan");
// The weighting record of a plan or a sweep (include/mbd_hip.h mbd_weighting) as the handle keeps it.  check_weighting: the refusals
// the record alone decides, in the header's order, each naming the field, before any device access.  set: behind the handle's NULL,
// session and enable_demo checks (nullptr clears); makes room for the log — three arrays [P][cap], cap = Ndiffuse - 1 entries per
// plan (weigh_kernel's LDS window is the launching unit's to raise: mbd_plan_set_weighting).  begin(): a run, a phase call or a tick
// starts its log; slot(): where the next score step's entry goes (plan 0's; weigh_kernel adds plan k's stride), count advanced.
struct WeightingRec {
  bool has = false;
  WeighRec rec{};
  int P = 1, cap = 0, count = 0;
  DevBuf<float> d_temp, d_ess;
  DevBuf<int> d_kept;
  int set(const mbd_weighting* r, int device, int P_, int cap_, int N);
  void begin() { count = 0; }
  WeighLog slot() {
    if (count >= cap) count = 0;  // (never: no loop scores more than Ndiffuse - 1 steps; the log stays inside its buffers regardless)
    const int c = count++;
    return WeighLog{d_temp.get() + c, d_ess.get() + c, d_kept.get() + c, (long long)cap};
  }
  int peek(const mbd_env* env, int k, float* temp_out, float* ess_out, int32_t* kept_out, int capacity, int* count_out,
           const char* what) const;
};
int check_weighting(const mbd_weighting* rec);
// the refusal of a record beside a to-go record (who: how the refused record's messages begin, handle: "plan" / "sweep")
int refuse_beside_togo(const char* who, const char* handle = "plan");
// The elite record of a plan or of all the plans of a sweep (include/mbd_hip.h mbd_elites) as the handle keeps it, with what the two
// handles do alike.  The state of P plans (a plan: P = 1): the elites' rows E [P][rows][HNu], their returns R and source indices src
// [P][rows] (rows = max(n, 1)), the device words count [P], and the three device logs [P][log_cap], rings of log_cap entries (a
// scratch record of the mbd_debug_* entries: 1).  count never comes back to the host inside a loop: every kernel loads it.  steps:
// plan k's selections since its log began — host bookkeeping PER PLAN: in a sweep session's mixed tick the episodes that idle make no
// selection, and their logs stay a single session's.  check_elites: the refusals the record alone decides against the handle's
// Nsample, update_method and enable_demo, in the header's order, each naming the field — host arithmetic, before any device access.
// set: behind the handle's refusals (nullptr clears); waits for the device, makes room, and leaves the launch that empties the
// elites to the caller.  The launches a step or a tick makes are each unit's own, over this struct: the single and the batch
// kernels live in different units (mbd_plan.hip elite_table / elite_inject / elite_select; mbd_sweep.hip likewise, with mask and strides).
struct EliteRec {
  bool has = false;
  int n = 0, nominal = 0, carry = 0, rows = 1, P = 1;
  int log_cap = kLogCap;
  long long steps[MBD_SWEEP_MAX_PLANS] = {};
  DevBuf<float> d_E, d_R, d_log_top;
  DevBuf<int> d_src, d_count, d_log_count, d_log_kept;
  void restart() { for (long long& c : steps) c = 0; }  // (the logs begin)
  void layout(int n_elites, int nominal_, int carry_, int P_) {
    n = n_elites; nominal = nominal_; carry = carry_; P = P_;
    rows = n > 0 ? n : 1;
  }
  MBD_HIDDEN int set(const mbd_elites* rec, int P_, int HNu, int device);
  // the scratch record of the mbd_debug_* entries: every buffer with all bits set, logs one entry long, count_in [P_] in the count
  // words and plan k's first count_in[k] rows from E_in [P_][rows][HNu] (NULL: none)
  MBD_HIDDEN int scratch(int n_elites, int nominal_, int P_, int HNu, const float* E_in, const int32_t* count_in);
  // HOST plan k's elites, their count and the most recent min(steps, capacity, log_cap) log entries, oldest first
  MBD_HIDDEN int peek(const mbd_env* env, int k, int HNu, float* elites_out, float* returns_out, int32_t* src_out, int32_t* count_out,
                      int32_t* log_count, int32_t* log_kept, float* log_top, int capacity, int* n_log_out, const char* what) const;
};
MBD_HIDDEN int check_elites(const mbd_elites* rec, int Nsample, int update_method, int enable_demo);
// the refusals the mbd_debug_elites_* entries share (mbd_records.hip: the host entry; mbd_plan.hip: the two that launch step kernels)
MBD_HIDDEN inline int check_elites_args(const char* what, const float* cand, int N, int HNu, const float* ybar, float sigma, int lazy, int n_elites,
                             int nominal, const float* E_in, int count_in) {
  if (!cand || !ybar) return fail(MBD_ERR_INVALID, "%s: NULL argument", what);
  if (N < 1 || HNu < 1 || (uint64_t)N * (uint64_t)HNu > (1ull << 26)) return fail(MBD_ERR_INVALID, "%s: N=%d HNu=%d", what, N, HNu);
  if (n_elites < 0 || n_elites > kEliteMax) return fail(MBD_ERR_INVALID, "%s: n_elites=%d outside [0, %d]", what, n_elites, kEliteMax);
  if (nominal != 0 && nominal != 1) return fail(MBD_ERR_INVALID, "%s: nominal=%d: 0 or 1", what, nominal);
  if (n_elites + nominal >= N) return fail(MBD_ERR_INVALID, "%s: n_elites=%d + nominal=%d must lie below N=%d", what, n_elites, nominal, N);
  if (count_in < 0 || count_in > n_elites) return fail(MBD_ERR_INVALID, "%s: count=%d outside [0, n_elites=%d]", what, count_in, n_elites);
  if (count_in > 0 && !E_in) return fail(MBD_ERR_INVALID, "%s: count=%d without elites", what, count_in);
  if (lazy && !(sigma > 0.0f)) return fail(MBD_ERR_INVALID, "%s: sigma=%g: a lazy plan's sigma is > 0", what, (double)sigma);
  return MBD_OK;
}
// The to-go record of a plan or of all the plans of a sweep (include/mbd_hip.h mbd_togo) as the handle keeps it: the record, the
// layout it gives at the handle's Hsample — G groups, group j's first row starts[j] = j block —, and the last step's returns and
// weights R, W [P][G][N] (row 0 of a plan's W is never written: group 0's weights are the plan's d_weights).  check_togo: the refusals
// the record alone decides against the handle's Hsample, Nsample, update_method and enable_demo, likewise.  set: behind the handle's
// refusals (nullptr clears); R and W read as all-ones bits until a step has run.  The step's two launches are each unit's own
// (togo_launch), and set stepped.
struct TogoRec {
  bool has = false;
  int block = 0, min_tail = 0, G = 0;
  bool stepped = false;  // a step of the record has run: d_weights are group 0's
  std::vector<int32_t> starts;
  DevBuf<float> d_R, d_W;
  MBD_HIDDEN void layout(int block_, int min_tail_, int H);  // the layout a record gives at horizon H
  MBD_HIDDEN int set(const mbd_togo* rec, int P, int H, int N, int device);
  // HOST starts [G], plan k's R and W [G][N]; d_weights: the handle's own [P][N], group 0's once a step of the record has written them
  MBD_HIDDEN int peek(const mbd_env* env, int k, int N, const float* d_weights, int32_t* starts_out, float* R_out, float* W_out,
                      int32_t* n_groups_out, const char* what) const;
};
constexpr int kTogoMaxN = 12288;  // the N weights of a group in the default 48 KB LDS window
MBD_HIDDEN int check_togo(const mbd_togo* rec, int Hsample, int Nsample, int update_method, int enable_demo);
// the refusals mbd_debug_togo_host (mbd_records.hip) and mbd_debug_togo_step (mbd_plan.hip: it launches step kernels) share
MBD_HIDDEN int check_togo_args(const char* what, int N, int H, int block, int min_tail);
// The pick record of a plan or a sweep (include/mbd_hip.h mbd_mpc_pick) as the handle keeps it, with what the two handles do alike.
// check_mpc_pick: the refusals the record alone decides, each naming the field, before any device access.  set: behind the handle's
// NULL, session, enable_demo and ensemble checks (nullptr clears); makes room for P plans' slots [P][3][HNu], their returns and
// per-step rewards.  start: in front of an episode's or a session's first tick — room for the log, a ring of min(n_ticks,
// kLogCap) entries per plan, entry of tick j at j % cap — and no tick served.  tick: the three launches (four with an objective
// record) behind a tick's last update kernel, on stream s; what it reads
// is PickTick, and it leaves P_t where M_t lay.  peek: the most recent min(count, capacity, cap) ticks of plan k, oldest first.
struct PickTick {
  const float* state;   // [P][S] where the tick planned from
  int N;                // candidates per plan
  const float* rews;    // [P][N] the rewards the last step's score read
  const float* cand;    // [P][N][HNu] the last step's candidates, or their normals (lazy) ...
  bool lazy;
  float sigma;          // ... with that step's sigma_i and Ybar_i
  const float* ybar_i;
  long long ybar_i_stride;
  float* M;             // the tick's result: P_t afterwards
  long long M_stride;
  const float* B;       // the Ybar the tick started from
  long long B_stride;
  unsigned cold;        // bit k: plan k's tick was cold
};
struct PickRec {
  bool has = false;
  int mask = 0, P = 1, HNu = 0, H = 0, cap = 0;
  long long count = 0;  // ticks served since start
  DevBuf<float> d_slots, d_rets, d_rewss, d_obj_ret, d_obj_cost, d_log_rets;
  DevBuf<int> d_best, d_log_choice, d_log_best;
  int set(const mbd_mpc_pick* rec, int device, int P_, int HNu_, int H_);
  int start(long long n_ticks);
  int tick(mbd_env* env, ObjectiveRec& obj, const ValueRec& val, const PickTick& tk, hipStream_t s);
  int peek(const mbd_env* env, int k, int32_t* choice_out, float* rets_out, int32_t* best_out, int capacity, int* count_out,
           const char* what) const;
};
int check_mpc_pick(const mbd_mpc_pick* rec);
// A step's candidates as the launches behind its sampler are handed them (an adapt record's update, an elite record's injection
// and selection): cand [N][HNu], or their normals (lazy) with the sigma_i and Ybar_i the step sampled with — an mppi plan's sigma
// from the carried device scalar, which its sampler read (d_sigma, nullptr: the host value).
struct StepCand {
  const float* cand;
  int N, HNu, lazy;
  float sigma;
  const float* d_sigma;
  const float* ybar_i;
};
// The plan-only record, in the form of the others: set behind the handle's refusals (nullptr clears), the launches a step or
// a tick makes — each returns at once without a record, and the mbd_debug_* entries run the same members on a scratch record —, and
// peek.  All zero: no record (a zeroed stand-in handle has none).
// The adapt record (include/mbd_hip.h mbd_adapt): the rule, the table a and G = a * g [HNu] on the device — G is what the samplers
// take as their shape while the record is in force (noise_spec) —, the scratch the update's two kernels hand var and s through, and
// the device log, a ring of kLogCap entries (count: steps since the log began).  g_cur: the caller's shape G was last formed under
// (the plan's d_shape or nullptr), which the update's second kernel forms G' under again.
struct AdaptRec {
  bool has = false;
  AdaptRule rule{};
  int carry = 0;
  long long count = 0;
  const float* g_cur = nullptr;
  DevBuf<float> d_a, d_G, d_buf, d_log_S;
  DevBuf<int> d_log_skipped;
  // g: the caller's shape in force outside warm ticks; the table is all ones afterwards (one launch on s, waited for)
  MBD_HIDDEN int set(const mbd_adapt* rec, int HNu, const float* g, const mbd_env* env, hipStream_t s);
  // The table at the start of a run or a tick, or under a new shape: shift < 0: a = ones, otherwise a shifted `shift` elements
  // forward (0: as it is); G = a * g under the caller's shape g now in force, which the updates that follow keep forming G under.
  // ONE launch.
  MBD_HIDDEN int table(int shift, const float* g, int HNu, hipStream_t s);
  // behind a step's update kernel, on the step's stream, from the step's weights d_w [N]: var into d_buf, then S, a', G' and the
  // log entry.  TWO launches; the weights are staged in LDS while they fit the default 48 KB window, read from memory beyond
  MBD_HIDDEN int update(const float* d_w, const StepCand& c, hipStream_t s);
  // HOST a_out [HNu] and the most recent min(count, capacity, kLogCap) log entries, oldest first
  MBD_HIDDEN int peek(const mbd_env* env, int HNu, float* a_out, float* ratio_out, int32_t* skipped_out, int capacity, int* count_out) const;
};
// the refusals the record alone decides against the handle's update_method and enable_demo, in the header's order, each naming the
// field — host arithmetic, before any device access
MBD_HIDDEN int check_adapt(const mbd_adapt* rec, int update_method, int enable_demo);
// One tick of a plant's disturbance chain, dk, d_t = split(dk): advances dk, fills slot k of sp with d_t and the record's
// deviations — the kick's only in the ticks that end with one — and says whether tick t does
bool plant_tick_draw(const mbd_mpc_plant& pr, int prng_impl, int t, uint32_t dk[2], SweepPlant& sp, int k);
