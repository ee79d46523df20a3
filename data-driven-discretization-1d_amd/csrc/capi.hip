// C ABI of libddd1d.so (include/ddd1d.h): model lifecycle, weight packing for
// the MFMA kernels, launch dispatch.  No torch types, no exceptions across the
// boundary.
#include <hip/hip_runtime.h>

#include <emmintrin.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/ddd1d.h"
#include "capi_common.h"
#include "dev_params.h"
#include "launch.h"
#include "launch_weno.h"
#include "ops.h"
#include "pack_device.h"
#include "pack_weights.h"
#ifdef DDD_PROBES
#include "probe_kernels.h"
#endif
#include "rhs_generic.h"
#include "rhs_lean.h"
#include "rhs_mfma.h"
#include "rhs_spectral.h"
#include "rhs_stream.h"
#include "ring_args.h"
#include "rollout_scores.h"
#include "rhs_weno.h"   // (host side only: weno::supports; the kernels are weno_unit.hip)

// What capi_train.hip shares (capi_common.h)
namespace ddd {
namespace capi {

thread_local std::string g_error;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}

bool is_conservative(int eq) {
  switch (eq) {
    case DDD_EQ_BURGERS_CONSERVATIVE: case DDD_EQ_KDV_CONSERVATIVE:
    case DDD_EQ_KS_CONSERVATIVE: case DDD_EQ_BURGERS_GODUNOV:
    case DDD_EQ_KDV_GODUNOV: case DDD_EQ_KS_GODUNOV:
      return true;
    default:
      return false;
  }
}

bool is_forced_family(int eq) {   // equations.py:276-277: only Burgers adds forcing(t)
  return eq == DDD_EQ_BURGERS || eq == DDD_EQ_BURGERS_CONSERVATIVE ||
         eq == DDD_EQ_BURGERS_GODUNOV;
}

}  // namespace capi
}  // namespace ddd

using namespace ddd::capi;

namespace {

// Profiling / A-B switches.  The product library (libddd1d.so) has none: the
// struct below is constant there and every test on it folds away.  In
// libddd1d_probe.so (-DDDD_PROBES, __graft_entry__.build_probe, used only by
// profiles/tools/ and `bench.py --debug-option`) they are set ONLY through
// ddd_debug_set_option (an explicit call that logs to stderr), never read from
// the environment: a stray variable must not be able to change the numerics
// path, skip kernel phases or hand the kernel a raw address.
struct DebugOptions {
  int no_fold = 0;       // keep the projection out of the output layer (D <= 2 models)
  int no_spec = 0;       // run-time-parameterised kernels instead of the per-equation ones
  int no_stream = 0;     // per-sample kernels instead of the streaming fixed-stencil kernel
  int no_lean = 0;       // the MFMA-path kernels (tower skipped) instead of rhs_lean.h
  int no_weno = 0;       // the generic kernel instead of rhs_weno.h
  int no_fft = 0;        // spectral models: the O(N^2) circulant form at every N
  int no_half = 0;       // nets of <= 16 filters: embedded in 32 instead of the 16-channel tiles
  int prio_split = 0;    // A/B: static wave priorities
  int stagger = 0;       // A/B: initial s_sleep of odd wave slots
  int substep_parts = 0; // A/B: sample slabs advanced side by side in the per-substep modes (0: auto)
  int ablate = 0;        // skips kernel phases: WRONG RESULTS (run-time-parameterised kernels)
  unsigned long long trace_ptr = 0;   // device buffer for s_memtime phase stamps
  unsigned long long walk_trace_ptr = 0;   // device buffer for the wave-lifetime stamps of the substep walk
};
#ifdef DDD_PROBES
DebugOptions g_debug;
#else
constexpr DebugOptions g_debug{};
#endif

template <typename T>
int upload(const std::vector<T>& host, T** dev) {
  *dev = nullptr;
  if (host.empty()) return DDD_OK;
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(dev), host.size() * sizeof(T)));
  DDD_HIP(hipMemcpy(*dev, host.data(), host.size() * sizeof(T),
                    hipMemcpyHostToDevice));
  return DDD_OK;
}

int expected_derivatives(int eq) {
  switch (eq) {
    case DDD_EQ_BURGERS: case DDD_EQ_BURGERS_CONSERVATIVE: case DDD_EQ_KDV:
    case DDD_EQ_KDV_CONSERVATIVE:
      return 2;
    case DDD_EQ_KS: case DDD_EQ_KS_CONSERVATIVE: case DDD_EQ_BURGERS_GODUNOV:
    case DDD_EQ_KDV_GODUNOV:
      return 3;
    case DDD_EQ_KS_GODUNOV:
      return 4;
    default:
      return -1;
  }
}

// b weights in float64 (the float32 tableau rounds 2/9, 1/3, 4/9, 1/6).
void tableau_weights_f64(int scheme, double (&b)[ddd::kMaxStages]) {
  for (double& v : b) v = 0.0;
  switch (scheme) {
    case DDD_SCHEME_EULER: b[0] = 1.0; break;
    case DDD_SCHEME_MIDPOINT: b[1] = 1.0; break;
    case DDD_SCHEME_BS3: b[0] = 2.0 / 9.0; b[1] = 1.0 / 3.0; b[2] = 4.0 / 9.0; break;
    case DDD_SCHEME_RK4: b[0] = 1.0 / 6.0; b[1] = 1.0 / 3.0; b[2] = 1.0 / 3.0; b[3] = 1.0 / 6.0; break;
    default: break;
  }
}

int make_tableau(int scheme, ddd::Tableau* tab) {
  std::memset(tab, 0, sizeof(*tab));
  switch (scheme) {
    case DDD_SCHEME_EULER:
      tab->stages = 1; tab->b[0] = 1.0f;
      return DDD_OK;
    case DDD_SCHEME_MIDPOINT:   // tf.contrib.integrate.odeint_fixed 'midpoint'
      tab->stages = 2;
      tab->a[1] = 0.5f; tab->c[1] = 0.5;
      tab->b[0] = 0.0f; tab->b[1] = 1.0f;
      return DDD_OK;
    case DDD_SCHEME_BS3:        // Bogacki-Shampine (SciPy RK23 tableau)
      tab->stages = 3;
      tab->a[1] = 0.5f; tab->a[2] = 0.75f;
      tab->c[1] = 0.5; tab->c[2] = 0.75;
      tab->b[0] = (float)(2.0 / 9.0); tab->b[1] = (float)(1.0 / 3.0);
      tab->b[2] = (float)(4.0 / 9.0);
      return DDD_OK;
    case DDD_SCHEME_RK4:
      tab->stages = 4;
      tab->a[1] = 0.5f; tab->a[2] = 0.5f; tab->a[3] = 1.0f;
      tab->c[1] = 0.5; tab->c[2] = 0.5; tab->c[3] = 1.0;
      tab->b[0] = (float)(1.0 / 6.0); tab->b[1] = (float)(1.0 / 3.0);
      tab->b[2] = (float)(1.0 / 3.0); tab->b[3] = (float)(1.0 / 6.0);
      return DDD_OK;
    default:
      return fail(DDD_ERR_INVALID_ARGUMENT, "unknown scheme %d", scheme);
  }
}

// The per-stage products of a fixed-step launch in the kernels' own arithmetic (float
// state: a[s] * (float)dt in float32; float64 state: (double)a[s] * dt; stage times
// c[s] * dt in float64) -- dev_params.h: StageConsts.
ddd::StageConsts make_stage_consts(const ddd::Tableau& tab, double dt) {
  ddd::StageConsts sc{};
  const float h = (float)dt;
  for (int s = 0; s < ddd::kMaxStages; ++s) {
    const volatile float ah = tab.a[s] * h, bh = tab.b[s] * h;   // (volatile: one rounding each,
    const volatile double ahd = (double)tab.a[s] * dt;            //  no host-side contraction)
    const volatile double bhd = (double)tab.b[s] * dt, ct = tab.c[s] * dt;
    sc.ah[s] = ah; sc.bh[s] = bh; sc.ahd[s] = ahd; sc.bhd[s] = bhd; sc.ct[s] = ct;
    if (s < tab.stages && tab.b[s] != 0.0f) sc.b_nonzero |= 1 << s;
  }
  return sc;
}

// Host side of the device-resident command ring (dev_params.h: RingArgs; rhs_mfma.h:
// substep_ring_kernel).  The caller's thread posts commands; a park thread (one per model that
// ever used the ring) posts kRingStop when the region has been idle for `idle` -- a caller
// that synchronises the device, or enqueues other work behind the persistent kernel, inside
// an open region waits that long, not for ever; the next ddd_rk_substep starts the kernel again.
struct Ring {
  void* slots = nullptr;         // page-locked, device-visible: [kRingSlots][kRingSlotChunks] x 16 B
  unsigned* done = nullptr;      // page-locked: [kRingSlots], written by the kernel
  unsigned* status = nullptr;    // page-locked: [0] watchdog expired
  unsigned* d_count = nullptr;   // device: [kRingSlots] + the relay lock
  void* d_slots = nullptr;       // device (fine-grained): the relayed commands
  std::mutex mu;
  std::condition_variable cv;
  std::thread parker;
  bool quit = false;
  bool running = false;          // a substep_ring_kernel is waiting for commands on `stream`
  bool dead = false;             // the watchdog expired: results of the region are undefined
  hipStream_t stream = nullptr;
  unsigned long long next_index = 0;    // index of the next command
  unsigned long long launch_index = 0;  // first command of the running kernel
  int grid = 0;
  std::chrono::steady_clock::time_point last_post;
  std::chrono::microseconds idle{2000};
  unsigned watchdog_ms = 20000;
  unsigned long long launches = 0, commands = 0;   // statistics (ddd_region_stats)
};

// One 16-byte store per chunk (see dev_params.h): payload dwords 3 c .. 3 c + 2, then the tag.
void ring_write(Ring* rg, unsigned long long index, const unsigned (&payload)[3 * ddd::kRingChunks]) {
  const unsigned tag = (unsigned)(index + 1ull);
  __m128i* slot = reinterpret_cast<__m128i*>(rg->slots) +
                  (size_t)(index & (ddd::kRingSlots - 1)) * ddd::kRingSlotChunks;
  for (int c = 0; c < ddd::kRingChunks; ++c)
    _mm_store_si128(slot + c, _mm_set_epi32((int)tag, (int)payload[3 * c + 2],
                                            (int)payload[3 * c + 1], (int)payload[3 * c]));
}

// Room for command `index`: the command kRingSlots before it has been passed by every group
// (or belongs to a kernel that has ended).  False: no progress for 10 s.
bool ring_wait_room(Ring* rg, unsigned long long index) {
  if (index < (unsigned long long)ddd::kRingSlots) return true;
  const unsigned long long old = index - ddd::kRingSlots;
  // (no shortcut for commands of an earlier launch: that kernel may still be working through
  // them while the next one is already enqueued behind it)
  const volatile unsigned* flag = rg->done + (old & (ddd::kRingSlots - 1));
  const unsigned want = (unsigned)(old + 1ull);
  if (*flag == want) return true;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 0; *flag != want; ++spin) {
    _mm_pause();
    if ((spin & 0xfff) == 0xfff) {
      if (*reinterpret_cast<const volatile unsigned*>(rg->status) != 0u) return false;
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) return false;
    }
  }
  return true;
}

// (rg->mu held)  Ends the running kernel: kRingStop is a command like any other, every group
// leaves after the commands before it.
bool ring_stop_locked(Ring* rg) {
  if (!rg->running) return true;
  rg->running = false;
  const bool room = ring_wait_room(rg, rg->next_index);
  unsigned payload[3 * ddd::kRingChunks] = {};
  payload[14] = (unsigned)ddd::kRingStop;
  // (without room the slot is overwritten all the same: the kernel must end, and a region
  // that made no progress for 10 s is reported as failed)
  ring_write(rg, rg->next_index, payload);
  ++rg->next_index;
  if (!room) rg->dead = true;
  return room;
}

void ring_parker(Ring* rg) {
  std::unique_lock<std::mutex> lk(rg->mu);
  while (!rg->quit) {
    if (!rg->running) { rg->cv.wait(lk); continue; }
    const auto deadline = rg->last_post + rg->idle;
    if (std::chrono::steady_clock::now() >= deadline) { (void)ring_stop_locked(rg); continue; }
    rg->cv.wait_until(lk, deadline);
  }
}

// Geometry of the MFMA path.  rows: grid points per workgroup; wave_rows: per
// wavefront.  One free-running 64-row wavefront per workgroup when whole
// samples fit 64 rows (optionally split over two 32-row or four 16-row wavefronts),
// else 256 rows on four wavefronts with block barriers.
struct MfmaGeometry { int rows, wave_rows; };

// Which kernel a call runs (plan_launch): decided once per launch from the model, the
// operation and a few facts of the call's arguments, then launched as planned.  The model
// keeps the plan of its most recent launch (ddd_kernel_name).
enum class Op { substep, step, persistent, adaptive, ring };
enum class Route { spectral, stream_fixed, lean, weno, generic, mfma };
// 64-row MFMA groups on one, two (kSplit) or four (kQuad) wavefronts, or one wavefront on the
// 16-channel tiles of nets of up to 16 filters (Tile16Tower)
enum class Tile { one_wave, split, quad, half };

struct Plan {
  Op op = Op::substep;
  Route route = Route::generic;
  MfmaGeometry geo{64, 64};
  int eq = -1;                  // per-equation kernel id, or -1
  Tile tile = Tile::one_wave;
  bool traced = false;          // (probes) the phase-traced persistent integrator
  const char* name = nullptr;   // ddd_kernel_name; nullptr: no launch recorded
  // CallFacts::population: why the population form of the planned kernel does not exist
  // (nullptr: it does -- mfma_population.hip)
  const char* no_population = nullptr;
};

}  // namespace

struct ddd_model {
  ddd_config cfg;
  ddd::DevParams dp;
  bool mfma_ok = false;
  std::string mfma_reason;
  int kernel = DDD_KERNEL_GENERIC;   // resolved family
  int force_rows = 0;                // 0 = automatic; 64 / 32 (64 rows on two waves) / 256
  bool explicit_kernel = false;      // ddd_set_kernel chose a family (disables automatic variants)
  bool spec_folded = false;          // w_final4 (specialised kernels) holds the folded output layer
  Plan last_plan;                    // the most recent launch (cleared by ddd_set_kernel)
  int64_t fma_per_point = 0;
  // device allocations
  float* d_weights = nullptr;
  float* d_weights4 = nullptr;      // channel-padded copy for the generic kernel's LDS staging
  float* d_nullspace = nullptr;
  float* d_bias = nullptr;
  float* d_w_input = nullptr;
  float* d_w_hidden = nullptr;
  float* d_w_final4 = nullptr;
  size_t n_w_input = 0, n_w_hidden = 0, n_w_final4 = 0;   // floats of the three arrays above
  float* d_w_final4_rt = nullptr;
  float* d_w_final4_split = nullptr;
  float* d_w_quad = nullptr;
  float* d_w_final4_half = nullptr;   // output layer of a <= 16-filter net (rhs_mfma.h Tile16Tower)
  float* d_w_t16 = nullptr;           // its input and hidden layers as 16x16x4 A operands
  bool wide = false;                 // run-time kernels of the wide flavour (rhs_mfma.h kWide)
  int tower_k = 5, tower_cb = 1;     // conv tower the MFMA kernels carry the net in (rhs_mfma.h Tower)
  bool big() const { return tower_k != ddd::mfma::kKW || tower_cb != 1; }
  float4* d_frc = nullptr;
  float* d_sp = nullptr;
  float* d_trig = nullptr;
  unsigned char* d_runs = nullptr;
  // spectral (float64) models: ddd_spectral_create
  bool spectral = false;
  ddd::spectral::Params sp{};
  double* d_kernels = nullptr;
  double2* d_fft_mult = nullptr;      // FFT mode (rhs_spectral.h): multipliers [D][N] and
  double2* d_fft_twiddle = nullptr;   // the twiddle table [N / 2]
  double* d_scratch64 = nullptr;
  size_t scratch64_doubles = 0;
  // per-substep launch mode: the ensemble is advanced as two half-ensembles on two
  // internal streams, so that one half's launch boundary overlaps the other's
  // steady state (ddd_integrate_fixed)
  hipStream_t aux_stream[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
  // ddd_stream_fork .. ddd_stream_join: the same two chains kept alive ACROSS
  // ddd_rk_substep / ddd_time_derivative calls of a caller that owns the RK loop
  struct Chain {
    bool open = false;        // between ddd_stream_fork and ddd_stream_join
    bool forked = false;      // the internal streams are running ahead of `stream`
    hipStream_t stream = nullptr;
    int batch = 0, halves = 1;
    int half_batch[4] = {0, 0, 0, 0}, slab_first[4] = {0, 0, 0, 0};
  } chain;
  // ... or, for the per-equation one-wave kernels, ONE persistent kernel fed through a
  // device-resident command ring (Ring above)
  Ring* ring = nullptr;
  int region_mode = DDD_REGION_AUTO;
  // output times of ddd_integrate_adaptive_f64: a small ring of (page-locked host
  // copy, device copy) pairs, each released by an event recorded behind the launch
  // that reads it -- the entry point only enqueues (no host synchronisation unless
  // kTimeSlots calls are still in flight), on whatever stream each call names
  static constexpr int kTimeSlots = 4;
  struct TimeSlot {
    double* host = nullptr;    // hipHostMalloc
    double* dev = nullptr;
    size_t capacity = 0;
    hipEvent_t done = nullptr;
    bool in_flight = false;
  } time_slot[kTimeSlots];
  int next_time_slot = 0;
  // scratch for the per-substep launch mode
  float* d_scratch = nullptr;
  size_t scratch_floats = 0;
};

int ddd::capi::common_config_checks(const ddd_config* cfg) {
  if (cfg == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "cfg is NULL");
  if (cfg->struct_size != (int32_t)sizeof(ddd_config))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_config.struct_size = %d, library expects %d (ABI mismatch)",
                cfg->struct_size, (int)sizeof(ddd_config));
  const int nd = expected_derivatives(cfg->equation);
  if (nd < 0) return fail(DDD_ERR_INVALID_ARGUMENT, "unknown equation %d", cfg->equation);
  if (cfg->num_derivatives != nd)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "equation %d has %d spatial derivatives, got num_derivatives = %d",
                cfg->equation, nd, cfg->num_derivatives);
  if (cfg->num_points < 2)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_points = %d", cfg->num_points);
  if (!(cfg->dx > 0.0))
    return fail(DDD_ERR_INVALID_ARGUMENT, "dx must be positive");
  if (cfg->stencil_size < 1 || cfg->stencil_size > DDD_MAX_STENCIL)
    return fail(DDD_ERR_INVALID_ARGUMENT, "stencil_size = %d out of range [1, %d]",
                cfg->stencil_size, DDD_MAX_STENCIL);
  return DDD_OK;
}

namespace {

void free_dev(void* p) { if (p) (void)hipFree(p); }

// rhs_mfma.h replaces u / stddev by q' = fma(fma(-q, s, u), r, q), q = RN(u r),
// r = RN(1 / s).  True for every float32 u iff it is true for the 2^23
// significands of one binade (scaling u by a power of two scales q, the
// residual and q' exactly, away from under/overflow).  ~0.1 s, cached per value.
bool division_shortcut_is_exact(float s) {
  static std::vector<std::pair<float, bool>> cache;
  for (const auto& kv : cache)
    if (std::memcmp(&kv.first, &s, sizeof(s)) == 0) return kv.second;
  const float r = (float)(1.0 / (double)s);
  bool exact = std::isfinite(r) && r != 0.0f;
  for (uint32_t bits = 0x3f800000u; exact && bits < 0x40000000u; ++bits) {
    float u;
    std::memcpy(&u, &bits, sizeof(u));
    const float q = u * r;
    const float fast = std::fmaf(std::fmaf(-q, s, u), r, q);
    exact = fast == u / s;
  }
  cache.emplace_back(s, exact);
  return exact;
}

void fill_equation(const ddd_config& cfg, ddd::DevParams* dp) {
  std::memset(dp, 0, sizeof(*dp));
  dp->equation = cfg.equation;
  dp->N = cfg.num_points;
  dp->D = cfg.num_derivatives;
  dp->G = cfg.stencil_size;
  dp->eta = (float)cfg.eta;
  dp->stddev = (float)cfg.standard_deviation;
  dp->inv_stddev = (float)(1.0 / (double)dp->stddev);
  dp->exact_div = division_shortcut_is_exact(dp->stddev) ? 0 : 1;
  dp->inv_dx = (float)(1.0 / cfg.dx);
  dp->conservative = is_conservative(cfg.equation) ? 1 : 0;
}

// Projection tables zero-padded to the kernels' stencil columns for the
// MFMA-path epilogue; they travel inside DevParams (kernel-argument segment).
// `identity`: polynomial_accuracy_order = 0 on the wide kernels -- output channel
// G d + g IS coefficient g of derivative d (model.py:460-475), expressed as a
// projection with unit rows and zero bias so that the unfolded epilogue applies.
int upload_padded_tables(ddd_model* m, const float* nullspace, const float* bias,
                         bool identity = false) {
  ddd::DevParams& dp = m->dp;
  std::memset(dp.ns8, 0, sizeof(dp.ns8));
  std::memset(dp.bias8, 0, sizeof(dp.bias8));
  dp.dsel_bits = 0;
  dp.dsel_valid = 0;
  if (bias != nullptr)
    for (int d = 0; d < dp.D; ++d)
      for (int g = 0; g < dp.G; ++g) dp.bias8[d][g] = bias[d * dp.G + g];
  if (identity) {
    for (int d = 0; d < dp.D; ++d)
      for (int g = 0; g < dp.G; ++g) {
        const int c = d * dp.G + g;
        dp.dsel_bits |= (unsigned long long)d << (2 * c);
        dp.dsel_valid |= 1u << c;
        dp.ns8[c][g] = 1.0f;
      }
  } else if (nullspace != nullptr) {
    for (int d = 0; d < dp.D; ++d)
      for (int j = 0; j < dp.in_size[d]; ++j) {
        const int c = dp.in_start[d] + j;
        dp.dsel_bits |= (unsigned long long)d << (2 * c);
        dp.dsel_valid |= 1u << c;
        for (int g = 0; g < dp.G; ++g)
          dp.ns8[c][g] = nullspace[dp.ns_off[d] + j * dp.G + g];
      }
  }
  return DDD_OK;
}

// Reorder conv weights into MFMA A-operand order: pack_weights.h computes every layout and
// the folding decisions on the host; here the buffers are uploaded and DevParams written.
int pack_mfma_weights(ddd_model* m, const ddd::pack::NetLayout& net) {
  ddd::DevParams& dp = m->dp;
  ddd::pack::Input in{};
  in.L = dp.L; in.D = dp.D; in.G = dp.G; in.C_out = dp.C_out; in.cout0 = dp.cout[0];
  in.act = dp.act; in.target = dp.target; in.pao = dp.pao;
  in.in_start = dp.in_start; in.in_size = dp.in_size; in.ns8 = dp.ns8; in.bias8 = dp.bias8;
  in.wide = m->wide; in.tower_k = m->tower_k; in.tower_cb = m->tower_cb;
  in.no_fold = g_debug.no_fold != 0;
  in.net = net;
  const ddd::pack::Packed packed = ddd::pack::pack_weights(in);
  int rc = upload(packed.w_input, &m->d_w_input);
  if (!rc) rc = upload(packed.w_hidden, &m->d_w_hidden);
  if (!rc && packed.unsupported) rc = DDD_ERR_UNSUPPORTED;
  if (!rc) rc = upload(packed.w_final4_rt, &m->d_w_final4_rt);
  if (!rc) rc = upload(packed.w_final4, &m->d_w_final4);
  if (!rc) rc = upload(packed.w_final4_split, &m->d_w_final4_split);
  if (!rc) rc = upload(packed.w_quad, &m->d_w_quad);
  if (!rc) rc = upload(packed.w_final4_half, &m->d_w_final4_half);
  if (!rc) rc = upload(packed.w_t16, &m->d_w_t16);
  m->n_w_input = packed.w_input.size();
  m->n_w_hidden = packed.w_hidden.size();
  m->n_w_final4 = packed.w_final4.size();
  dp.w_input = m->d_w_input;
  dp.w_hidden = m->d_w_hidden;
  dp.w_final4_rt = m->d_w_final4_rt;
  dp.w_final4 = m->d_w_final4;
  dp.w_final4_split = m->d_w_final4_split;
  dp.w_quad = m->d_w_quad;
  dp.folded = packed.folded;
  dp.rt_groups = packed.rt_groups;
  dp.fin4_groups = packed.fin4_groups;
  m->spec_folded = packed.spec_folded;
  return rc;
}

// One-layer nets the MFMA-path kernels carry on their VALU route (DevParams::linear_taps).
bool linear_eligible(const ddd::DevParams& dp) {
  return !dp.fixed && dp.L == 1 && dp.target == ddd::TARGET_COEFFICIENTS &&
         !(dp.pao <= 0 && dp.unbiased) && dp.D <= 3 && dp.G <= ddd::kGMax && dp.K <= 7 &&
         dp.K * dp.D <= ddd::kChMax;
}

void decide_mfma(ddd_model* m) {
  const ddd::DevParams& dp = m->dp;
  char why[256] = "";
  bool ok = true;
  auto no = [&](const char* msg) { if (ok) snprintf(why, sizeof(why), "%s", msg); ok = false; };
  if (dp.N < 8 || dp.N > 256) no("num_points outside [8, 256]");
  if (dp.G > ddd::kGWide) no("stencil wider than 12");
  if (dp.G > dp.N) no("stencil wider than the grid");
  if (dp.fixed && dp.weno) no("WENO reconstruction");
  // The wide flavour of the run-time-parameterised kernels (stencils up to 12
  // points, up to 24 net output channels, projection folded into the output layer) carries what
  // the default flavour (8 points, 16 channels) cannot: coefficient_grid_min_size
  // = 9 and polynomial_accuracy_order = 0 with three derivatives
  // (training_test.py:56-57).
  bool wide = dp.G > ddd::kGMax;
  const bool linear = linear_eligible(dp);
  if (!dp.fixed && !linear) {
    // direct heads (space_derivatives / time_derivative / flux: D or 1 output
    // channels) and polynomial_accuracy_order = 0 (D x G coefficient channels,
    // no projection) run on the run-time-parameterised MFMA kernels
    if (dp.target == ddd::TARGET_COEFFICIENTS && dp.pao <= 0 && dp.D > 2) wide = true;
    if (dp.C_out > ddd::kChMax) wide = true;
    // the smallest tower built that holds the net (launch.h: DDD_FOR_EACH_BIG_TOWER + the
    // default 5 x 32); nets in between are packed zero-padded (pack_weights.h: embed_tower)
    m->tower_k = dp.K <= 3 ? 3 : dp.K <= 5 ? 5 : 7;
    m->tower_cb = dp.F <= 32 ? 1 : 2;
    if (m->tower_cb == 2 && m->tower_k == 3) m->tower_k = 5;   // (64-filter towers: 5 and 7 taps)
    // up to 16 filters of up to 3 taps in the architecture of the per-equation kernels: the
    // 5 x 32 tower, whose persistent integrators carry such nets on 16-channel tiles (rhs_mfma.h
    // Tile16Tower) -- ahead of the 3-tap tower, where they would occupy a quarter of every MFMA
    if (m->tower_k == 3 && dp.F <= 16 && dp.L == 3 && dp.act == ddd::ACT_RELU && !wide &&
        dp.target == ddd::TARGET_COEFFICIENTS && dp.pao > 0 &&
        dp.equation >= ddd::EQ_BURGERS && dp.equation <= ddd::EQ_KS_CONS &&
        dp.G == ddd::mfma::spec_stencil(dp.equation))
      m->tower_k = 5;
    if (dp.F > 64) no("filter_size > 64");
    if (dp.K > 7) no("kernel_size > 7");
    if (dp.L < 2) no("fewer than 2 conv layers");
    // the wide flavour folds every coefficient net into its output layer (pack_weights.h):
    // three derivatives' worth of register slots; the projection tables hold 24 net channels
    if (wide && dp.target == ddd::TARGET_COEFFICIENTS && dp.D > ddd::mfma::kWideDerivs)
      no("wide stencils / > 16 output channels with four derivatives");
    if (dp.C_out > ddd::kChWide && !(wide && dp.target == ddd::TARGET_COEFFICIENTS && dp.pao <= 0))
      no("more than 24 output channels");
    // stencils > 8 points / > 16 channels exist on the 5 x 32 tower only (wide flavour)
    if (wide && m->tower_k == 3) m->tower_k = 5;
    if (wide && m->big()) no("wide stencils / > 16 output channels with a tower other than 5 x 32");
  }
  if (!ok || dp.fixed || linear) { m->tower_k = 5; m->tower_cb = 1; }
  m->wide = ok && wide;
  m->mfma_ok = ok;
  m->mfma_reason = why;
  m->kernel = ok ? DDD_KERNEL_MFMA : DDD_KERNEL_GENERIC;
}

int check_generic_lds(const ddd_model* m, int state_bytes) {
  const size_t need = ddd::generic::lds_bytes(m->dp, state_bytes);
  if (need > 160 * 1024)
    return fail(DDD_ERR_UNSUPPORTED,
                "generic kernel needs %zu B of LDS per sample (limit 163840): "
                "num_points x channels too large", need);
  return DDD_OK;
}

int ensure_scratch(ddd_model* m, size_t floats) {
  if (m->scratch_floats >= floats) return DDD_OK;
  free_dev(m->d_scratch);
  m->d_scratch = nullptr;
  m->scratch_floats = 0;
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(&m->d_scratch), floats * sizeof(float)));
  m->scratch_floats = floats;
  return DDD_OK;
}

int check_batch(const ddd_model* m, int batch, bool want_spectral = false) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (m->spectral != want_spectral)
    return fail(DDD_ERR_UNSUPPORTED,
                m->spectral ? "spectral (float64) models only accept the *_f64 entry points"
                            : "this entry point needs a spectral model (ddd_spectral_create)");
  if (batch < 0) return fail(DDD_ERR_INVALID_ARGUMENT, "negative batch");
  if (m->dp.forced && batch > m->dp.forcing_batch)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "batch %d exceeds the %d samples forcing was set for", batch,
                m->dp.forcing_batch);
  return DDD_OK;
}

// One-time hardware check of the DPP wavefront rotate the one-wave kernel uses
// for the flux exchange when N = 64 (falls back to ds_bpermute otherwise).
int dpp_wave_rol_ok() {
  static int ok = -1;
  if (ok >= 0) return ok;
  ok = 0;
  float* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), 64 * sizeof(float)) != hipSuccess) return ok;
  hipLaunchKernelGGL(ddd::ops::dpp_rotate_probe_kernel, dim3(1), dim3(64), 0, nullptr, d);
  float h[64];
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
    ok = 1;
    for (int l = 0; l < 64; ++l)
      if (h[l] != (float)(((l + 1) % 64) * 3 + 1)) ok = 0;
  }
  (void)hipFree(d);
  return ok;
}

int device_simds() {
  static int simds = 0;
  if (simds == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      simds = prop.multiProcessorCount * 4;
    if (simds <= 0) simds = 1024;
  }
  return simds;
}

MfmaGeometry mfma_geometry(const ddd_model* m) {
  const bool fits64 = m->dp.N <= 64 && 64 % m->dp.N == 0;
  if (m->force_rows == 256 || !fits64) return {256, 64};
  if (m->force_rows == 64) return {64, 64};
  if (m->force_rows == 32 && !m->wide && !m->big()) return {64, 32};   // (no wide / other-tower split)
  if (m->force_rows == 16 && !m->wide && !m->big()) return {64, 16};
  return {64, 64};
}

// Workgroups of `batch` samples in geometry geo ...
int group_count(const ddd_model* m, MfmaGeometry geo, int batch) {
  const int spg = geo.rows / m->dp.N;
  return (batch + spg - 1) / spg;
}

// ... and how many of them the machine holds resident (the grid of the kernels that walk
// over several groups: substep_multi_kernel, step_multi_kernel, the command ring).
int resident_groups(MfmaGeometry geo) {
  return geo.rows == 64 ? 2 * device_simds() : device_simds() / 2;
}

// Equation id of the compile-time specialised integrator this model can use,
// or -1: the default architecture (three relu conv layers, default stencil
// width, projection folded when D <= 2) on a non-Godunov equation.
int spec_equation(const ddd_model* m, int rows) {
  const ddd::DevParams& dp = m->dp;
  if (g_debug.no_spec || m->wide || m->big()) return -1;
  if (dp.forced) {
    // the specialised kernels only carry the harmonic-sum forcing (rhs_mfma.h:
    // launch_setup `fast`); exotic tables go to the run-time kernels
    const int spg = rows / dp.N;
    const bool fast = spg * dp.P <= rows && dp.n_k <= 6 &&
                      spg * ddd::mfma::kTrigMax <= 3 * rows / 4 && dp.P < 256;
    if (!fast) return -1;
  }
  if (dp.fixed || dp.L != 3 || dp.act != ddd::ACT_RELU) return -1;
  if (dp.target != ddd::TARGET_COEFFICIENTS || dp.pao <= 0) return -1;
  if (dp.equation < ddd::EQ_BURGERS || dp.equation > ddd::EQ_KS_CONS) return -1;
  if (dp.D != ddd::mfma::spec_derivs(dp.equation)) return -1;
  if (dp.G != ddd::mfma::spec_stencil(dp.equation)) return -1;
  if ((dp.conservative != 0) != ddd::mfma::spec_flux_form(dp.equation)) return -1;
  // the kernels hard-wire the null-space split (rhs_mfma.h: spec_in_size) and
  // whether their packed output layer is folded
  int start = 0;
  for (int d = 0; d < dp.D; ++d) {
    if (dp.in_size[d] != ddd::mfma::spec_in_size(dp.equation, d) || dp.in_start[d] != start)
      return -1;
    start += dp.in_size[d];
  }
  if (m->spec_folded != ddd::mfma::spec_folded(dp.equation)) return -1;
  return dp.equation;
}

bool aligned16(const void* ptr) {
  return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0;
}

// WENO5 + Godunov-flux models (integrate.WENODifferentiator, the exact Burgers solver) on
// the one-wavefront-per-sample kernels of rhs_weno.h; an explicit ddd_set_kernel(GENERIC)
// keeps the generic kernel (A/B, and the grids rhs_weno.h does not carry).
bool use_weno_kernel(const ddd_model* m) {
  return m->kernel == DDD_KERNEL_GENERIC && !m->explicit_kernel && !g_debug.no_weno &&
         ddd::weno::supports(m->dp);
}

// The persistent kernels of fixed-stencil models and one-layer nets (rhs_lean.h) built, one
// per taps x derivatives: f(taps, derivatives) as integral constants for dp's; false when
// there is none (other tap counts: the MFMA-path kernels with the tower skipped).
template <int kK, int kD, typename F>
bool lean_kernel_if(int taps, int derivs, F& f) {
  if (taps != kK || derivs != kD) return false;
  f(std::integral_constant<int, kK>{}, std::integral_constant<int, kD>{});
  return true;
}
template <typename F>
bool with_lean_kernel(const ddd::DevParams& dp, F&& f) {
  if (!ddd::lean::supports(dp)) return false;
  const int t = dp.fixed ? 0 : dp.linear_taps, d = dp.D;
  return lean_kernel_if<0, 1>(t, d, f) || lean_kernel_if<0, 2>(t, d, f) ||
         lean_kernel_if<0, 3>(t, d, f) || lean_kernel_if<0, 4>(t, d, f) ||
         lean_kernel_if<3, 1>(t, d, f) || lean_kernel_if<3, 2>(t, d, f) ||
         lean_kernel_if<3, 3>(t, d, f) || lean_kernel_if<5, 1>(t, d, f) ||
         lean_kernel_if<5, 2>(t, d, f) || lean_kernel_if<5, 3>(t, d, f) ||
         lean_kernel_if<7, 1>(t, d, f) || lean_kernel_if<7, 2>(t, d, f);
}

// f(EQ) as an integral constant: the launch.h templates of the per-equation kernels.
template <typename F>
void with_equation(int eq, F&& f) {
  switch (eq) {
    case ddd::EQ_BURGERS: f(std::integral_constant<int, ddd::EQ_BURGERS>{}); break;
    case ddd::EQ_BURGERS_CONS: f(std::integral_constant<int, ddd::EQ_BURGERS_CONS>{}); break;
    case ddd::EQ_KDV: f(std::integral_constant<int, ddd::EQ_KDV>{}); break;
    case ddd::EQ_KDV_CONS: f(std::integral_constant<int, ddd::EQ_KDV_CONS>{}); break;
    case ddd::EQ_KS: f(std::integral_constant<int, ddd::EQ_KS>{}); break;
    case ddd::EQ_KS_CONS: f(std::integral_constant<int, ddd::EQ_KS_CONS>{}); break;
    default: break;
  }
}

template <typename F>
void with_rows(int rows, F&& f) {
  if (rows == 64) f(std::integral_constant<int, 64>{});
  else f(std::integral_constant<int, 256>{});
}

// f(taps, 32-channel blocks, rows) as integral constants for the model's tower other than
// 5 taps x 32 channels (launch.h: DDD_FOR_EACH_BIG_TOWER).
template <typename F>
void with_big_tower(const ddd_model* m, int rows, F&& f) {
#define DDD_BIG_TOWER(K, CB)                                                     \
  if (m->tower_k == K && m->tower_cb == CB)                                      \
    with_rows(rows, [&](auto r) {                                                \
      f(std::integral_constant<int, K>{}, std::integral_constant<int, CB>{}, r); \
    });
  DDD_FOR_EACH_BIG_TOWER(DDD_BIG_TOWER)
#undef DDD_BIG_TOWER
}

const char* plan_name(const Plan& p) {
  switch (p.route) {
    case Route::spectral: return "spectral_f64";
    case Route::stream_fixed: return "stream_fixed";
    case Route::lean: return "valu_f32_lean";
    case Route::weno: return "valu_f32_weno";
    case Route::generic: return "generic";
    case Route::mfma: break;
  }
  if (p.geo.rows == 256) return "mfma_f32_r256";
  switch (p.tile) {
    case Tile::quad: return "mfma_f32_r64w16";
    case Tile::half: return "mfma_f32_r64h16";
    case Tile::split: return "mfma_f32_r64w32";
    default: return "mfma_f32_r64";
  }
}

// What the rules read of a call's arguments.
struct CallFacts {
  int batch = 0;
  bool f64 = false;       // float64 state
  bool views = false;     // derivative or coefficient views requested
  bool coeffs = false;    // ... coefficients (the WENO kernels write none)
  bool aligned = false;   // every state array 16-byte aligned (the streaming kernels)
  // a replica population in one launch (ddd_population_*): the machine is filled by
  // replicas x groups, so none of the small-ensemble geometries; Plan::no_population says
  // whether the kernel planned has a population form
  bool population = false;
};

CallFacts substep_facts(const ddd::SubstepArgs& a) {
  return {a.batch, false, a.derivs_out != nullptr || a.coeffs_out != nullptr, a.coeffs_out != nullptr,
          aligned16(a.y_in) && aligned16(a.y_base) && aligned16(a.y_out) &&
              aligned16(a.acc_in) && aligned16(a.acc_out)};
}

// Geometry, per-equation kernel and tile of an MFMA launch.
void plan_mfma(const ddd_model* m, const CallFacts& f, Plan* p) {
  const bool automatic = !m->explicit_kernel;
  MfmaGeometry geo = mfma_geometry(m);
  int eq = -1;
  switch (p->op) {
    case Op::substep:
    case Op::ring:
      if (geo.wave_rows == 16) geo = {64, 64};   // (four-wavefront groups: integrators only)
      // per-equation instantiations for the plain substep (no derivative views)
      if (!f.views && geo.wave_rows == 64) eq = spec_equation(m, geo.rows);
      break;
    case Op::step:
      if (automatic) eq = spec_equation(m, geo.rows);
      break;
    case Op::persistent:
      if (geo.rows == 64 && geo.wave_rows == 64 && !f.f64 && automatic && !f.population &&
          m->dp.w_final4_split != nullptr && spec_equation(m, 64) >= 0) {
        // small ensembles: two 32-row wavefronts per sample (rhs_mfma.h kSplit)
        // measured (profiles/r4_ablation.txt, N = 64): B = 256: 1.63 x the one-wavefront kernel (twice
        // the SIMDs busy), B = 512: 0.97 x, B = 1024: 0.89 x (two coupled wavefronts per SIMD lose to one
        // free-running one) -- so only below three eighths of a wavefront per SIMD
        const int groups = group_count(m, geo, f.batch);
        if (8 * groups <= 3 * device_simds()) geo = {64, 32};
        // ... and FOUR 16-row wavefronts per group (kQuad: every layer on 16x16x4 MFMAs, one
        // group on the four SIMDs of a CU) while that leaves at most two wavefronts per SIMD
        // (measured, profiles/r6_ablation.txt)
        if (m->dp.w_quad != nullptr && 2 * groups <= device_simds()) geo = {64, 16};
      }
      // an explicit DDD_KERNEL_MFMA_ROWS64_W16 where the model has no such kernel (float64
      // state, no per-equation specialisation): the one-wavefront geometry
      if (geo.wave_rows == 16 && !(!f.f64 && m->dp.w_quad != nullptr && spec_equation(m, 64) >= 0))
        geo = {64, 64};
      // per-equation instantiations: 64-row wavefronts in both geometries and both state types,
      // the split and quad groups for float32 state
      if (geo.wave_rows != 32 || (!f.f64 && m->dp.w_final4_split != nullptr))
        eq = spec_equation(m, geo.rows);
#ifdef DDD_PROBES
      if (g_debug.trace_ptr != 0) {
        // phase tracing: the dedicated traced instantiation (headline config) or
        // the run-time-parameterised kernel
        p->traced = eq == ddd::EQ_BURGERS_CONS && geo.rows == 64 && !f.f64;
        if (!p->traced) eq = -1;
      }
#endif
      break;
    case Op::adaptive: {
      // the two-wave split has no adaptive instantiation.  Small ensembles: every 64-row group
      // on four 16-row wavefronts (rhs_mfma.h kQuad), as for the fixed-step integrators --
      // the reference's callers integrate tens to hundreds of samples
      // (scripts/run_evaluation.py:212-221)
      const bool want_quad = geo.rows == 64 && !f.population &&
                             (geo.wave_rows == 16 || (geo.wave_rows == 64 && m->force_rows == 0));
      if (geo.wave_rows != 64) geo = {64, 64};
      eq = spec_equation(m, geo.rows);
      if (want_quad && m->dp.w_quad != nullptr && eq >= 0 &&
          (m->force_rows == 16 ||
           (automatic && 2 * group_count(m, geo, f.batch) <= device_simds())))
        geo = {64, 16};
      break;
    }
  }
  p->geo = geo;
  p->eq = eq;
  p->tile = geo.wave_rows == 32 ? Tile::split : geo.wave_rows == 16 ? Tile::quad : Tile::one_wave;
  // nets of up to 16 filters: the 16-channel tiles of the per-equation one-wave kernels
  if (p->tile == Tile::one_wave && geo.rows == 64 && eq >= 0 && !p->traced &&
      m->d_w_final4_half != nullptr && m->d_w_t16 != nullptr &&
      !g_debug.no_half)
    p->tile = Tile::half;
}

// The one place that chooses a launch's kernel.  Order: spectral, the streaming
// fixed-stencil kernels, the lean kernel (persistent float32 integrator), MFMA, WENO,
// generic.  Op::step plans a kernel that takes all stages of a step; without one the
// plan's op is Op::substep (one launch per substep, each planned on its own).  Op::ring
// plans the command ring's persistent kernel; when the call cannot ride the ring, the plan
// is the one of Op::substep.
Plan plan_launch(const ddd_model* m, Op op, const CallFacts& f) {
  Plan p;
  p.op = op;
  const bool automatic = !m->explicit_kernel;
  if (op == Op::ring) {
    // per-equation kernels on one-wave groups (N | 64), the whole ensemble from sample 0, no
    // derivative / coefficient views; opt-in (measured equal to the launches)
    p = plan_launch(m, Op::substep, f);
    if (m->region_mode == DDD_REGION_RING && automatic && f.batch > 0 &&
        p.route == Route::mfma && p.geo.rows == 64 && p.eq >= 0) {
      p.op = Op::ring;
      p.tile = Tile::one_wave;   // (the ring kernel carries the net on the 32-channel tower)
      p.name = plan_name(p);
    }
    return p;
  }
  if (m->spectral) {
    p.route = Route::spectral;
  } else if (automatic && !g_debug.no_stream && f.aligned && !f.views &&
             (op == Op::substep ? ddd::stream::supports(m->dp)
                                : op == Op::step && ddd::stream::step_supports(m->dp))) {
    // fixed-stencil models without forcing: the streaming kernels (rhs_stream.h)
    p.route = Route::stream_fixed;
  } else if (m->kernel == DDD_KERNEL_MFMA) {
    // fixed stencils / one-layer nets, float32 state, whole samples per wavefront: the
    // lane == grid point kernel (no matrix work to schedule around)
    if (op == Op::persistent && !f.f64 && automatic && !g_debug.no_lean &&
        with_lean_kernel(m->dp, [](auto, auto) {})) {
      p.route = Route::lean;
    } else {
      p.route = Route::mfma;
      plan_mfma(m, f, &p);
    }
  } else if (use_weno_kernel(m) && !f.coeffs) {
    p.route = Route::weno;
  }
  if (op == Op::step && p.route != Route::stream_fixed && !(p.route == Route::mfma && p.eq >= 0))
    p.op = Op::substep;
  p.name = plan_name(p);
  if (f.population) {
    // the population forms built: the per-equation one-wavefront integrators, float32 fixed
    // step and adaptive (launch.h: integrate_population_spec, adaptive_population_spec)
    if (!automatic) p.no_population = "an explicit ddd_set_kernel choice";
    else if (op != Op::persistent && op != Op::adaptive)
      p.no_population = "only the persistent launch mode and the adaptive integrator";
    else if (p.route != Route::mfma) p.no_population = "the model is not on the MFMA route";
    else if (p.geo.rows != 64 || p.geo.wave_rows != 64)
      p.no_population = "num_points does not divide 64 (four-wavefront 256-row geometry)";
    else if (p.eq < 0)
      p.no_population = "no per-equation specialisation (run-time-parameterised, wide or "
                        "other-tower kernels)";
    else if (p.tile != Tile::one_wave)
      p.no_population = "nets of up to 16 filters run on the 16-channel-tile kernels";
    else if (op == Op::persistent && f.f64) p.no_population = "float64 fixed-step state";
    // (probe build: the population launches carry neither the phase stamps nor the A/B knobs
    // that launch_integrate hands the solo kernels)
    else if (p.traced) p.no_population = "phase tracing is on (probe library)";
  }
  return p;
}

// The parameters of one launch: the model's, with the forcing rows of its sample slab
// (sample0: first sample of the launch in the model's per-sample tables) and the weights
// of its tile.
ddd::DevParams launch_params(ddd_model* m, const Plan& p, int sample0 = 0) {
  if (p.route == Route::mfma) m->dp.dpp_rol = dpp_wave_rol_ok();
  ddd::DevParams dp = m->dp;
  if (sample0 != 0 && dp.forced) {
    dp.frc += (size_t)sample0 * dp.P;
    dp.runs += (size_t)sample0 * 8;
  }
  if (p.tile == Tile::half) {
    dp.w_final4 = m->d_w_final4_half;
    dp.w_quad = m->d_w_t16;
  }
  return dp;
}

// sample0: index of a.y_in's first sample in the model's per-sample tables (a
// half-ensemble launch); grid_share: this launch may occupy 1 / grid_share of
// the machine-sized grid (it runs next to grid_share - 1 others).
int launch_substep(ddd_model* m, const Plan& p, const ddd::SubstepArgs& a, hipStream_t stream,
                   int sample0 = 0, int grid_share = 1) {
  if (a.batch == 0) return DDD_OK;
  m->last_plan = p;
  if (p.route == Route::stream_fixed) {
    const long pts = (long)ddd::stream::samples_per_block(m->dp.N) * m->dp.N;
    const long total = (long)a.batch * m->dp.N;
    const unsigned blocks = (unsigned)((total + pts - 1) / pts);
    ddd::stream::launch_fixed_substep(dim3(blocks), stream, m->dp, a);
  } else if (p.route == Route::mfma) {
    const ddd::DevParams dp = launch_params(m, p, sample0);
    const int blocks = group_count(m, p.geo, a.batch);
    // specialised models: machine-sized grid, weights resident per wavefront,
    // each group walks over several row groups (substep_multi_kernel)
    const int grid = std::min(blocks, resident_groups(p.geo) / std::max(grid_share, 1));
    if (p.eq >= 0) {
      with_equation(p.eq, [&](auto eq) {
        if (p.tile == Tile::half)
          ddd::launch::substep_half_spec<decltype(eq)::value>(dp, a, blocks, grid, stream);
        else
          ddd::launch::substep_spec<decltype(eq)::value>(p.geo.rows, dp, a, blocks, grid, stream);
      });
    } else if (m->big()) {
      with_big_tower(m, p.geo.rows, [&](auto k, auto cb, auto rows) {
        ddd::launch::substep_big_unit<decltype(k)::value, decltype(cb)::value, decltype(rows)::value>(
            dp, a, blocks, stream);
      });
    } else if (m->wide) {
      with_rows(p.geo.rows, [&](auto rows) {
        ddd::launch::substep_wide_unit<decltype(rows)::value>(dp, a, blocks, stream);
      });
    } else {
      ddd::launch::substep_runtime(p.geo.rows, p.geo.wave_rows, dp, a, blocks, stream);
    }
  } else if (p.route == Route::weno) {
    ddd::launch::weno_substep(launch_params(m, p, sample0), a, stream);
  } else {
    int rc = check_generic_lds(m, 0);
    if (rc) return rc;
    const size_t lds = ddd::generic::lds_bytes(m->dp, 0);
    DDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ddd::generic::substep_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ddd::generic::substep_kernel, dim3(a.batch),
                       dim3(ddd::generic::kThreads), lds, stream, m->dp, a);
  }
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

Plan plan_substep(const ddd_model* m, const ddd::SubstepArgs& a) {
  return plan_launch(m, Op::substep, substep_facts(a));
}

template <typename ST>
int launch_integrate(ddd_model* m, const Plan& p, ddd::IntegrateArgs a, hipStream_t stream) {
  if (a.batch == 0 || a.n_steps == 0) return DDD_OK;
  m->last_plan = p;
#ifdef DDD_PROBES   // profiling knobs (ddd_debug_set_option; profiles/r1_ablation.txt)
  a.prio_split = g_debug.prio_split;
  a.stagger = g_debug.stagger;
  a.trace = reinterpret_cast<unsigned long long*>(g_debug.trace_ptr);
  a.ablate = g_debug.ablate;
#endif
  constexpr bool f64 = std::is_same<ST, double>::value;
  if (p.route == Route::lean) {
    // one instantiation per (taps, derivatives, stencil-column pairs)
    const int blocks = group_count(m, {64, 64}, a.batch);
    with_lean_kernel(m->dp, [&](auto k, auto d) {
      constexpr int K = decltype(k)::value, D = decltype(d)::value;
      if (ddd::lean::column_pairs(m->dp.G) == 3)
        hipLaunchKernelGGL((ddd::lean::integrate_kernel<K, D, 3>), dim3(blocks), dim3(64), 0, stream, m->dp, a);
      else
        hipLaunchKernelGGL((ddd::lean::integrate_kernel<K, D, 4>), dim3(blocks), dim3(64), 0, stream, m->dp, a);
    });
  } else if (p.route == Route::mfma) {
    const ddd::DevParams dp = launch_params(m, p);
    const int blocks = group_count(m, p.geo, a.batch);
    const bool hoist = !m->dp.fixed && m->dp.L == 3;
    if (p.eq >= 0) {
      with_equation(p.eq, [&](auto eq) {
        constexpr int EQ = decltype(eq)::value;
        switch (p.tile) {
          case Tile::half:
            if (f64) ddd::launch::integrate_half_f64_spec<EQ>(dp, a, blocks, stream);
            else ddd::launch::integrate_half_spec<EQ>(dp, a, blocks, stream);
            break;
          case Tile::quad: ddd::launch::integrate_quad_spec<EQ>(dp, a, blocks, stream); break;
          case Tile::split: ddd::launch::integrate_split_spec<EQ>(dp, a, blocks, stream); break;
          default: ddd::launch::integrate_spec<EQ>(p.geo.rows, f64, p.traced, dp, a, blocks, stream);
        }
      });
    } else if (m->big()) {
      with_big_tower(m, p.geo.rows, [&](auto k, auto cb, auto rows) {
        ddd::launch::integrate_big_unit<decltype(k)::value, decltype(cb)::value,
                                        decltype(rows)::value, f64>(dp, a, blocks, stream);
      });
    } else if (m->wide) {
      with_rows(p.geo.rows, [&](auto rows) {
        ddd::launch::integrate_wide_unit<decltype(rows)::value, f64 ? 1 : 0>(hoist, dp, a, blocks,
                                                                            stream);
      });
    } else {
      ddd::launch::integrate_runtime(p.geo.rows, p.geo.wave_rows, f64, hoist, dp, a, blocks, stream);
    }
  } else if (p.route == Route::weno) {
    ddd::launch::weno_integrate(f64, m->dp, a, stream);
  } else {
    int rc = check_generic_lds(m, (int)sizeof(ST));
    if (rc) return rc;
    const size_t lds = ddd::generic::lds_bytes(m->dp, (int)sizeof(ST));
    DDD_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(ddd::generic::integrate_kernel<ST>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((ddd::generic::integrate_kernel<ST>), dim3(a.batch),
                       dim3(ddd::generic::kThreads), lds, stream, m->dp, a);
  }
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int check_integrate_args(const ddd_model* m, int n_steps, int save_every,
                         const void* y0, const void* y_out, int batch) {
  int rc = check_batch(m, batch);
  if (rc) return rc;
  if (n_steps < 0) return fail(DDD_ERR_INVALID_ARGUMENT, "negative n_steps");
  if (save_every < 1) return fail(DDD_ERR_INVALID_ARGUMENT, "save_every must be >= 1");
  if (batch > 0 && n_steps > 0 && (y0 == nullptr || y_out == nullptr))
    return fail(DDD_ERR_INVALID_ARGUMENT, "y0 / y_out is NULL");
  return DDD_OK;
}

// Large ensembles on the per-equation MFMA kernels are advanced as TWO
// half-ensembles (contiguous sample slabs, independent of each other) on two
// internal streams, each launch sized to half the machine: while one half is at
// a kernel boundary (drain, dispatch, 29 KB of weights per wavefront before the
// first MFMA) the other half's wavefronts have the matrix pipes to themselves,
// which a single wavefront per SIMD nearly saturates.  Still one fused launch per
// substep for every sample; results are bit-identical (same kernel, same
// arithmetic).  Used by ddd_integrate_fixed (per-substep / per-step modes) and,
// across calls, by ddd_rk_substep / ddd_time_derivative inside a
// ddd_stream_fork .. ddd_stream_join region.
constexpr int kMaxParts = 4;
struct SlabPlan {
  int halves = 1;                                 // slabs advanced side by side
  int half_batch[kMaxParts] = {0, 0, 0, 0};
  int slab_first[kMaxParts] = {0, 0, 0, 0};       // first sample of each slab
};

SlabPlan plan_slabs(const ddd_model* m, int batch) {
  SlabPlan plan;
  plan.half_batch[0] = batch;
  if (m->kernel != DDD_KERNEL_MFMA || m->explicit_kernel || g_debug.no_spec) return plan;
  const MfmaGeometry geo = mfma_geometry(m);
  const int groups = group_count(m, geo, batch);
  if (geo.wave_rows != 64 || spec_equation(m, geo.rows) < 0 || groups < 2 * resident_groups(geo))
    return plan;
  plan.halves = 2;
  if (g_debug.substep_parts > 0) plan.halves = std::min(g_debug.substep_parts, kMaxParts);
  const int per = ((groups + plan.halves - 1) / plan.halves) * (geo.rows / m->dp.N);   // whole workgroups
  int first = 0;
  for (int i = 0; i < plan.halves; ++i) {
    plan.slab_first[i] = first;
    plan.half_batch[i] = std::max(0, std::min(per, batch - first));
    first += plan.half_batch[i];
  }
  return plan;
}

// The internal streams start after everything already enqueued on `stream` ...
int fork_lanes(ddd_model* m, hipStream_t stream, int halves) {
  for (int i = 0; i < halves; ++i) {
    if (m->aux_stream[i] == nullptr)
      DDD_HIP(hipStreamCreateWithFlags(&m->aux_stream[i], hipStreamNonBlocking));
    if (m->ev_join[i] == nullptr)
      DDD_HIP(hipEventCreateWithFlags(&m->ev_join[i], hipEventDisableTiming));
  }
  if (m->ev_fork == nullptr)
    DDD_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
  DDD_HIP(hipEventRecord(m->ev_fork, stream));
  for (int i = 0; i < halves; ++i) DDD_HIP(hipStreamWaitEvent(m->aux_stream[i], m->ev_fork, 0));
  // (No start offset between the chains: whatever it is, they settle into the
  // same steady state within a few launches -- measured 0 .. 1.75 half-launches,
  // 72.4 +- 0.1 % throughout, profiles/r3_ablation.txt.)
  return DDD_OK;
}

// ... and `stream` continues after everything enqueued on them.  Never skipped: an
// error inside a forked region still joins before it is reported.
int join_lanes(ddd_model* m, hipStream_t stream, int halves) {
  for (int i = 0; i < halves; ++i) {
    DDD_HIP(hipEventRecord(m->ev_join[i], m->aux_stream[i]));
    DDD_HIP(hipStreamWaitEvent(stream, m->ev_join[i], 0));
  }
  return DDD_OK;
}

// Entry points other than ddd_rk_substep / ddd_time_derivative end a caller's
// chained region (ddd_stream_fork) before they touch the model: its stream then
// sees every substep enqueued so far.
int chain_close(ddd_model* m) {
  int rc = DDD_OK;
  if (m->ring != nullptr) {
    std::lock_guard<std::mutex> lk(m->ring->mu);
    if (!ring_stop_locked(m->ring))
      rc = fail(DDD_ERR_HIP, "command ring: the persistent kernel made no progress for 10 s");
  }
  if (m->chain.open && m->chain.forked && m->chain.halves > 1)
    rc = join_lanes(m, m->chain.stream, m->chain.halves);
  m->chain.open = false;
  m->chain.forked = false;
  return rc;
}

int ring_create(ddd_model* m) {
  Ring* rg = new Ring();
  const size_t slot_bytes = (size_t)ddd::kRingSlots * ddd::kRingSlotChunks * 16;
  hipError_t err = hipHostMalloc(&rg->slots, slot_bytes, hipHostMallocCoherent | hipHostMallocMapped);
  if (err == hipSuccess)
    err = hipHostMalloc(reinterpret_cast<void**>(&rg->done), (ddd::kRingSlots + 32 + 2048) * sizeof(unsigned),
                        hipHostMallocCoherent | hipHostMallocMapped);
  if (err == hipSuccess)
    err = hipMalloc(reinterpret_cast<void**>(&rg->d_count), (ddd::kRingSlots + 16) * sizeof(unsigned));
  if (err == hipSuccess)   // fine-grained: every XCD's L2 sees the relaying wavefront's stores
    err = hipExtMallocWithFlags(&rg->d_slots, slot_bytes, hipDeviceMallocFinegrained);
  if (err == hipSuccess)   // (every slot's last group resets its count; the relay lock starts open)
    err = hipMemset(rg->d_count, 0, (ddd::kRingSlots + 16) * sizeof(unsigned));
  if (err == hipSuccess) err = hipMemset(rg->d_slots, 0, slot_bytes);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    if (rg->slots) (void)hipHostFree(rg->slots);
    if (rg->done) (void)hipHostFree(rg->done);
    if (rg->d_count) (void)hipFree(rg->d_count);
    if (rg->d_slots) (void)hipFree(rg->d_slots);
    delete rg;
    return fail(DDD_ERR_HIP, "command ring: %s", hipGetErrorString(err));
  }
  std::memset(rg->slots, 0, slot_bytes);
  std::memset(rg->done, 0, (ddd::kRingSlots + 32 + 2048) * sizeof(unsigned));   // (+ status, trace stamps)
  rg->status = rg->done + ddd::kRingSlots;
  rg->parker = std::thread(ring_parker, rg);
  m->ring = rg;
  return DDD_OK;
}

void ring_destroy(ddd_model* m) {
  Ring* rg = m->ring;
  if (rg == nullptr) return;
  {
    std::lock_guard<std::mutex> lk(rg->mu);
    (void)ring_stop_locked(rg);
    rg->quit = true;
  }
  rg->cv.notify_all();
  rg->parker.join();
  // the kernel reads the ring until it ends (a stream the caller has already destroyed: the device)
  if (rg->stream == nullptr || hipStreamSynchronize(rg->stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
  }
  (void)hipHostFree(rg->slots);
  (void)hipHostFree(rg->done);
  (void)hipFree(rg->d_count);
  (void)hipFree(rg->d_slots);
  delete rg;
  m->ring = nullptr;
}

// One command = one ddd_rk_substep call (p: a plan of Op::ring).  Starts the persistent
// kernel when none is waiting.
int ring_post(ddd_model* m, const Plan& p, const ddd::SubstepArgs& a, hipStream_t stream) {
  if (m->ring == nullptr) { int rc = ring_create(m); if (rc) return rc; }
  Ring* rg = m->ring;
  std::unique_lock<std::mutex> lk(rg->mu);
  if (rg->dead || *reinterpret_cast<const volatile unsigned*>(rg->status) != 0u) {
    rg->dead = true; rg->running = false;
    return fail(DDD_ERR_HIP, "command ring: the persistent kernel gave up waiting (watchdog) or "
                             "made no progress; the region's results are undefined");
  }
  if (rg->running && rg->stream != stream) (void)ring_stop_locked(rg);
  if (!rg->running) {
    const ddd::DevParams dp = launch_params(m, p);
    rg->grid = std::min(group_count(m, p.geo, a.batch), resident_groups(p.geo));
    ddd::RingArgs r{};
    r.slots = rg->slots; r.dev_slots = rg->d_slots; r.count = rg->d_count; r.done = rg->done; r.status = rg->status;
    r.first_index = (unsigned)rg->next_index;
    r.watchdog_ticks = rg->watchdog_ms * 100000u;   // 100 MHz
    with_equation(p.eq, [&](auto eq) {
      ddd::launch::substep_ring_spec<decltype(eq)::value>(dp, r, rg->grid, stream);
    });
    DDD_HIP(hipGetLastError());
    rg->running = true;
    rg->stream = stream;
    rg->launch_index = rg->next_index;
    ++rg->launches;
    rg->last_post = std::chrono::steady_clock::now();
    rg->cv.notify_all();
  }
  if (!ring_wait_room(rg, rg->next_index)) {
    rg->dead = true;
    (void)ring_stop_locked(rg);
    return fail(DDD_ERR_HIP, "command ring: the persistent kernel made no progress for 10 s");
  }
  unsigned payload[3 * ddd::kRingChunks] = {};
  const auto put64 = [&](int j, unsigned long long v) {
    payload[j] = (unsigned)v; payload[j + 1] = (unsigned)(v >> 32);
  };
  unsigned long long tbits; std::memcpy(&tbits, &a.t, 8);
  put64(0, tbits);
  put64(2, (unsigned long long)(uintptr_t)a.y_in);
  put64(4, (unsigned long long)(uintptr_t)a.y_base);
  put64(6, (unsigned long long)(uintptr_t)a.y_out);
  put64(8, (unsigned long long)(uintptr_t)a.acc_in);
  put64(10, (unsigned long long)(uintptr_t)a.acc_out);
  std::memcpy(&payload[12], &a.c1, 4);
  std::memcpy(&payload[13], &a.c2, 4);
  payload[14] = (unsigned)a.batch;
  ring_write(rg, rg->next_index, payload);
  ++rg->next_index;
  ++rg->commands;
  rg->last_post = std::chrono::steady_clock::now();
  m->last_plan = p;
  return DDD_OK;
}

// One substep of a caller-owned Runge-Kutta loop.  Outside a chained region: one
// launch on the caller's stream.  Inside (same stream): slab i of this call is
// ordered after slab i of the previous call only -- the two half-ensemble chains
// of ddd_integrate_fixed, kept alive across calls.
int substep_entry(ddd_model* m, const ddd::SubstepArgs& a, hipStream_t stream) {
  ddd_model::Chain& ch = m->chain;
  if (!ch.open || stream != ch.stream || a.derivs_out != nullptr || a.coeffs_out != nullptr)
    return launch_substep(m, plan_substep(m, a), a, stream);
  const Plan p = plan_launch(m, Op::ring, substep_facts(a));
  if (p.op == Op::ring) {
    if (ch.forked && ch.halves > 1) {   // (a region that started on the two chains)
      int rc = join_lanes(m, stream, ch.halves);
      ch.forked = false;
      if (rc) return rc;
    }
    return ring_post(m, p, a, stream);
  }
  if (m->ring != nullptr) {   // this call takes launches: behind every command posted so far
    std::lock_guard<std::mutex> lk(m->ring->mu);
    (void)ring_stop_locked(m->ring);
  }
  if (!ch.forked || ch.batch != a.batch) {
    if (ch.forked && ch.halves > 1) {   // another batch: other slabs, so join first
      int rc = join_lanes(m, stream, ch.halves);
      if (rc) return rc;
    }
    const SlabPlan plan = plan_slabs(m, a.batch);
    ch.batch = a.batch;
    ch.halves = plan.halves;
    for (int i = 0; i < kMaxParts; ++i) {
      ch.half_batch[i] = plan.half_batch[i];
      ch.slab_first[i] = plan.slab_first[i];
    }
    ch.forked = true;
    if (ch.halves > 1) {
      int rc = fork_lanes(m, stream, ch.halves);
      if (rc) { ch.forked = false; return rc; }
    }
  }
  if (ch.halves <= 1) return launch_substep(m, p, a, stream);
  int rc = DDD_OK;
  for (int hf = 0; hf < ch.halves && rc == DDD_OK; ++hf) {
    if (ch.half_batch[hf] == 0) continue;
    const size_t off = (size_t)ch.slab_first[hf] * m->dp.N;
    ddd::SubstepArgs h = a;
    h.batch = ch.half_batch[hf];
    h.y_in = a.y_in + off;
    if (a.y_base != nullptr) h.y_base = a.y_base + off;
    if (a.y_out != nullptr) h.y_out = a.y_out + off;
    if (a.acc_in != nullptr) h.acc_in = a.acc_in + off;
    if (a.acc_out != nullptr) h.acc_out = a.acc_out + off;
    rc = launch_substep(m, plan_substep(m, h), h, m->aux_stream[hf], ch.slab_first[hf], ch.halves);
  }
  if (rc) {   // do not leave the internal streams running ahead of a failed call
    (void)join_lanes(m, stream, ch.halves);
    ch.forked = false;
  }
  return rc;
}

}  // namespace

extern "C" {

int ddd_abi_version(void) { return DDD_ABI_VERSION; }

const char* ddd_last_error(void) { return g_error.c_str(); }

int ddd_scheme_stages(int scheme) {
  ddd::Tableau tab;
  if (make_tableau(scheme, &tab) != DDD_OK) return -1;
  return tab.stages;
}

int ddd_model_create(const ddd_config* cfg, const float* weights, size_t n_weights,
                     const float* nullspace, size_t n_nullspace, const float* bias,
                     size_t n_bias, ddd_model** out) {
  if (out == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  int rc = common_config_checks(cfg);
  if (rc) return rc;
  if (cfg->num_layers < 1 || cfg->num_layers > DDD_MAX_LAYERS)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "num_layers = %d out of range [1, %d] (fold num_layers = 0 models "
                "into ddd_baseline_create)", cfg->num_layers, DDD_MAX_LAYERS);
  if (cfg->filter_size < 1 || cfg->kernel_size < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "filter_size / kernel_size must be >= 1");
  if (cfg->activation < DDD_ACT_RELU || cfg->activation > DDD_ACT_ELU)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown activation %d", cfg->activation);
  if (cfg->model_target < DDD_TARGET_COEFFICIENTS || cfg->model_target > DDD_TARGET_FLUX)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown model_target %d", cfg->model_target);
  if (!(cfg->standard_deviation > 0.0))
    return fail(DDD_ERR_INVALID_ARGUMENT, "standard_deviation must be positive");
  if (weights == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "weights is NULL");

  ddd_model* m = new ddd_model();
  m->cfg = *cfg;
  fill_equation(*cfg, &m->dp);
  ddd::DevParams& dp = m->dp;
  dp.fixed = 0;
  dp.target = cfg->model_target;
  dp.L = cfg->num_layers;
  dp.F = cfg->filter_size;
  dp.K = cfg->kernel_size;
  dp.act = cfg->activation;
  dp.pao = cfg->polynomial_accuracy_order;
  dp.unbiased = cfg->ensure_unbiased_coefficients;

  const bool projected = dp.target == ddd::TARGET_COEFFICIENTS && dp.pao > 0;
  int c_out = 1;
  if (dp.target == ddd::TARGET_COEFFICIENTS) {
    if (projected) {
      c_out = 0;
      for (int d = 0; d < dp.D; ++d) {
        if (cfg->input_sizes[d] < 1 || cfg->input_sizes[d] > dp.G) {
          delete m;
          return fail(DDD_ERR_INVALID_ARGUMENT, "input_sizes[%d] = %d out of range [1, G]",
                      d, cfg->input_sizes[d]);
        }
        dp.in_start[d] = c_out;
        dp.in_size[d] = cfg->input_sizes[d];
        dp.ns_off[d] = c_out * dp.G;
        c_out += cfg->input_sizes[d];
      }
    } else {
      c_out = dp.D * dp.G;
    }
  } else if (dp.target == ddd::TARGET_SPACE_DERIVATIVES) {
    c_out = dp.D;
  }
  dp.C_out = c_out;

  size_t off = 0;
  int64_t fma = 0;
  for (int l = 0; l < dp.L; ++l) {
    dp.cin[l] = l == 0 ? 1 : dp.F;
    dp.cout[l] = l == dp.L - 1 ? c_out : dp.F;
    dp.w_off[l] = (int)off;
    off += (size_t)dp.K * dp.cin[l] * dp.cout[l];
    dp.b_off[l] = (int)off;
    off += (size_t)dp.cout[l];
    fma += (int64_t)dp.K * dp.cin[l] * dp.cout[l];
  }
  if (n_weights != off) {
    delete m;
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "n_weights = %zu, configuration needs %zu floats", n_weights, off);
  }
  if (dp.target == ddd::TARGET_COEFFICIENTS) {
    if (projected) for (int d = 0; d < dp.D; ++d) fma += (int64_t)dp.in_size[d] * dp.G;
    fma += (int64_t)dp.D * dp.G;
  }
  m->fma_per_point = fma;

  if (projected) {
    if (nullspace == nullptr || bias == nullptr || n_nullspace != (size_t)c_out * dp.G ||
        n_bias != (size_t)dp.D * dp.G) {
      delete m;
      return fail(DDD_ERR_INVALID_ARGUMENT,
                  "nullspace/bias required: expected %zu and %zu floats, got %zu and %zu",
                  (size_t)c_out * dp.G, (size_t)dp.D * dp.G, n_nullspace, n_bias);
    }
  }

  std::vector<float> wv(weights, weights + n_weights);
  rc = upload(wv, &m->d_weights);
  dp.weights = m->d_weights;
  if (!rc) {
    // the generic kernel stages a layer's weights in LDS with the output channels
    // padded to fours ([K][cin][c4] + bias [c4]): kept in that form, so that the
    // staging is a straight float4 copy (rhs_generic.h)
    std::vector<float> w4;
    for (int l = 0; l < dp.L; ++l) {
      const int c4 = (dp.cout[l] + 3) & ~3;
      dp.w4_off[l] = (int)w4.size();
      const float* w = wv.data() + dp.w_off[l];
      const float* b = wv.data() + dp.b_off[l];
      for (int kc = 0; kc < dp.K * dp.cin[l]; ++kc)
        for (int col = 0; col < c4; ++col)
          w4.push_back(col < dp.cout[l] ? w[(size_t)kc * dp.cout[l] + col] : 0.0f);
      for (int col = 0; col < c4; ++col) w4.push_back(col < dp.cout[l] ? b[col] : 0.0f);
    }
    rc = upload(w4, &m->d_weights4);
    dp.weights4 = m->d_weights4;
  }
  if (!rc && projected) {
    std::vector<float> nv(nullspace, nullspace + n_nullspace);
    std::vector<float> bv(bias, bias + n_bias);
    rc = upload(nv, &m->d_nullspace);
    if (!rc) rc = upload(bv, &m->d_bias);
    dp.nullspace = m->d_nullspace;
    dp.bias = m->d_bias;
  }
  if (!rc) {
    decide_mfma(m);
    if (m->mfma_ok && linear_eligible(dp)) {
      // coeff[d][g] = B[d][g] + sum_k M[k][d][g] (u / std)[x + k - K/2]: the conv layer, the
      // null-space projection and the accuracy bias folded in float64, rounded once
      std::memset(dp.ns8, 0, sizeof(dp.ns8));
      std::memset(dp.bias8, 0, sizeof(dp.bias8));
      const float* w = wv.data() + dp.w_off[0];   // [K][1][C_out]
      const float* b = wv.data() + dp.b_off[0];
      for (int d = 0; d < dp.D; ++d)
        for (int g = 0; g < dp.G; ++g) {
          if (projected) {
            double acc = (double)bias[d * dp.G + g];
            for (int j = 0; j < dp.in_size[d]; ++j)
              acc += (double)b[dp.in_start[d] + j] * (double)nullspace[dp.ns_off[d] + j * dp.G + g];
            dp.bias8[d][g] = (float)acc;
            for (int k = 0; k < dp.K; ++k) {
              double mk = 0.0;
              for (int j = 0; j < dp.in_size[d]; ++j)
                mk += (double)w[(size_t)k * dp.C_out + dp.in_start[d] + j] *
                      (double)nullspace[dp.ns_off[d] + j * dp.G + g];
              dp.ns8[k * dp.D + d][g] = (float)mk;
            }
          } else {   // polynomial_accuracy_order 0: the layer emits the coefficients themselves
            dp.bias8[d][g] = b[d * dp.G + g];
            for (int k = 0; k < dp.K; ++k)
              dp.ns8[k * dp.D + d][g] = w[(size_t)k * dp.C_out + d * dp.G + g];
          }
        }
      dp.linear_taps = dp.K;
      dp.folded = 0;
      dp.dsel_bits = 0;
      dp.dsel_valid = 0;
    } else if (m->mfma_ok) {
      const bool fold_shape = dp.D <= 2 && dp.G >= 6 && dp.G <= ddd::kGMax && !m->wide;
      rc = upload_padded_tables(m, projected ? nullspace : nullptr, projected ? bias : nullptr,
                                dp.target == ddd::TARGET_COEFFICIENTS && !projected &&
                                    !fold_shape && !m->wide);
      if (!rc) {
        // (the generic kernel keeps the model's own K, F and weights: a model that
        // falls back to it -- N > 256, ddd_set_kernel(generic) -- never runs the
        // padded net; only the MFMA packing sees the embedding)
        std::vector<float> padded;
        ddd::pack::NetLayout net;
        net.weights = wv.data();
        for (int l = 0; l < dp.L; ++l) { net.w_off[l] = dp.w_off[l]; net.b_off[l] = dp.b_off[l]; }
        if (dp.K != m->tower_k || dp.F != 32 * m->tower_cb)
          ddd::pack::embed_tower(dp, wv, m->tower_k, 32 * m->tower_cb, &padded, &net);
        rc = pack_mfma_weights(m, net);
      }
    }
  }
  if (rc) { ddd_model_destroy(m); return rc; }
  *out = m;
  return DDD_OK;
}

int ddd_baseline_create(const ddd_config* cfg, const float* stencils, size_t n_stencils,
                        ddd_model** out) {
  if (out == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  int rc = common_config_checks(cfg);
  if (rc) return rc;
  if (stencils == nullptr ||
      n_stencils != (size_t)cfg->num_derivatives * cfg->stencil_size)
    return fail(DDD_ERR_INVALID_ARGUMENT, "stencils must hold D*G = %d floats, got %zu",
                cfg->num_derivatives * cfg->stencil_size, n_stencils);
  ddd_model* m = new ddd_model();
  m->cfg = *cfg;
  fill_equation(*cfg, &m->dp);
  m->dp.fixed = 1;
  m->dp.weno = cfg->weno_reconstruction != 0;
  if (m->dp.weno && (cfg->num_derivatives < 2 || cfg->equation < DDD_EQ_BURGERS_GODUNOV)) {
    delete m;
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "weno_reconstruction needs a Godunov-flux equation (u_minus, u_plus)");
  }
  m->dp.stddev = 1.0f;
  m->dp.inv_stddev = 1.0f;
  m->dp.exact_div = 0;
  m->fma_per_point = (int64_t)cfg->num_derivatives * cfg->stencil_size;
  std::vector<float> sv(stencils, stencils + n_stencils);
  rc = upload(sv, &m->d_bias);
  m->dp.bias = m->d_bias;
  if (!rc) {
    decide_mfma(m);
    // the padded stencil table also feeds the streaming kernel (any N <= 1024)
    if (m->mfma_ok || m->dp.G <= ddd::kGWide) rc = upload_padded_tables(m, nullptr, stencils);
  }
  if (rc) { ddd_model_destroy(m); return rc; }
  *out = m;
  return DDD_OK;
}

int ddd_spectral_create(const ddd_config* cfg, const double* kernels, size_t n_kernels,
                        ddd_model** out) {
  if (out == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  int rc = common_config_checks(cfg);
  if (rc) return rc;
  if (cfg->equation != DDD_EQ_BURGERS && cfg->equation != DDD_EQ_KDV &&
      cfg->equation != DDD_EQ_KS)
    return fail(DDD_ERR_UNSUPPORTED,
                "spectral models exist for the non-flux equations only (integrate.py:346)");
  if (cfg->num_points > ddd::spectral::kMaxPoints || cfg->num_points % 2)
    return fail(DDD_ERR_UNSUPPORTED, "spectral models need an even num_points <= %d (got %d)",
                ddd::spectral::kMaxPoints, cfg->num_points);
  if (kernels == nullptr || n_kernels != (size_t)cfg->num_derivatives * cfg->num_points)
    return fail(DDD_ERR_INVALID_ARGUMENT, "kernels must hold D*N = %d doubles, got %zu",
                cfg->num_derivatives * cfg->num_points, n_kernels);
  ddd_model* m = new ddd_model();
  m->cfg = *cfg;
  fill_equation(*cfg, &m->dp);
  m->spectral = true;
  m->kernel = DDD_KERNEL_GENERIC;
  m->mfma_reason = "spectral model";
  m->fma_per_point = (int64_t)cfg->num_derivatives * cfg->num_points;
  m->sp.equation = cfg->equation;
  m->sp.N = cfg->num_points;
  m->sp.D = cfg->num_derivatives;
  m->sp.eta = cfg->eta;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->d_kernels), n_kernels * sizeof(double));
  if (e == hipSuccess)
    e = hipMemcpy(m->d_kernels, kernels, n_kernels * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    ddd_model_destroy(m);
    return fail(DDD_ERR_HIP, "spectral kernels upload: %s", hipGetErrorString(e));
  }
  m->sp.kernels = m->d_kernels;
  // FFT mode for the large exact grids (N a power of two >= 512; rhs_spectral.h): the same
  // D circulant operators as diagonal multipliers in Fourier space, mult[d] = DFT(kernel[d]).
  // Formed HERE from the caller's kernels, so every Nyquist / sign convention of the call
  // that produced them carries over unchanged; a direct O(N^2) DFT in long double (once per
  // model: 12 M complex terms at N = 2048, D = 3), twiddles exp(-2 pi i m / N) likewise.
  const int n = cfg->num_points;
  if (n >= ddd::spectral::kFftMinPoints && (n & (n - 1)) == 0 && !g_debug.no_fft) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    std::vector<long double> cs(n), sn(n);
    for (int j = 0; j < n; ++j) {
      cs[j] = cosl(two_pi * (long double)j / (long double)n);
      sn[j] = sinl(two_pi * (long double)j / (long double)n);
    }
    std::vector<double2> mult((size_t)cfg->num_derivatives * n), tw(n / 2);
    for (int d = 0; d < cfg->num_derivatives; ++d)
      for (int k = 0; k < n; ++k) {
        long double re = 0.0L, im = 0.0L;
        for (int j = 0; j < n; ++j) {
          const int a = (int)(((long long)j * k) % n);
          const long double c = (long double)kernels[(size_t)d * n + j];
          re += c * cs[a];
          im -= c * sn[a];
        }
        mult[(size_t)d * n + k] = make_double2((double)re, (double)im);
      }
    for (int i = 0; i < n / 2; ++i) tw[i] = make_double2((double)cs[i], (double)-sn[i]);
    int rc2 = upload(mult, &m->d_fft_mult);
    if (rc2 == DDD_OK) rc2 = upload(tw, &m->d_fft_twiddle);
    if (rc2 != DDD_OK) { ddd_model_destroy(m); return rc2; }
    m->sp.fft_mult = m->d_fft_mult;
    m->sp.fft_twiddle = m->d_fft_twiddle;
    m->sp.fft_log2n = 31 - __builtin_clz((unsigned)n);
    m->fma_per_point = (int64_t)(2 + (cfg->num_derivatives + 1) / 2) * 5 * m->sp.fft_log2n / 2;
  }
  *out = m;
  return DDD_OK;
}

namespace {
int launch_spectral(ddd_model* m, const ddd::spectral::SubstepArgs64& a, hipStream_t stream) {
  if (a.batch == 0) return DDD_OK;
  const size_t lds = ddd::spectral::lds_bytes(m->sp);
  DDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ddd::spectral::substep_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ddd::spectral::substep_kernel, dim3(a.batch),
                     dim3(ddd::spectral::kThreads), lds, stream, m->sp, a);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}
}  // namespace

int ddd_time_derivative_f64(ddd_model* m, double t, const double* y, double* dydt, int batch,
                            void* stream) {
  (void)t;   // the equations of motion are autonomous; forcing stays on the host
  int rc = check_batch(m, batch, true);
  if (rc) return rc;
  if (batch > 0 && (!y || !dydt)) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  ddd::spectral::SubstepArgs64 a{};
  a.y_in = y; a.c1 = 1.0; a.y_out = dydt; a.batch = batch;
  return launch_spectral(m, a, static_cast<hipStream_t>(stream));
}

int ddd_rk_substep_f64(ddd_model* m, double t, const double* y_in, const double* y_base,
                       double c1, double* y_out, const double* acc_in, double c2,
                       double* acc_out, int batch, void* stream) {
  (void)t;
  int rc = check_batch(m, batch, true);
  if (rc) return rc;
  if (batch > 0 && !y_in) return fail(DDD_ERR_INVALID_ARGUMENT, "y_in is NULL");
  if (batch > 0 && !y_out && !acc_out)
    return fail(DDD_ERR_INVALID_ARGUMENT, "both y_out and acc_out are NULL");
  ddd::spectral::SubstepArgs64 a{};
  a.y_in = y_in; a.y_base = y_base; a.c1 = c1; a.y_out = y_out;
  a.acc_in = acc_in; a.c2 = c2; a.acc_out = acc_out; a.batch = batch;
  return launch_spectral(m, a, static_cast<hipStream_t>(stream));
}

int ddd_model_destroy(ddd_model* m) {
  if (m == nullptr) return DDD_OK;
  (void)chain_close(m);   // the caller's stream sees every substep before the buffers go
  ring_destroy(m);
  free_dev(m->d_weights); free_dev(m->d_weights4); free_dev(m->d_nullspace); free_dev(m->d_bias);
  free_dev(m->d_w_hidden);
  free_dev(m->d_w_input);
  free_dev(m->d_w_final4_half); free_dev(m->d_w_t16);
  free_dev(m->d_w_final4); free_dev(m->d_w_final4_rt); free_dev(m->d_w_final4_split); free_dev(m->d_w_quad); free_dev(m->d_frc); free_dev(m->d_sp); free_dev(m->d_trig);
  if (m->d_runs != nullptr) (void)hipFree(m->d_runs);
  free_dev(m->d_scratch);
  for (auto& slot : m->time_slot) {
    if (slot.done != nullptr) {
      if (slot.in_flight) (void)hipEventSynchronize(slot.done);
      (void)hipEventDestroy(slot.done);
    }
    if (slot.host != nullptr) (void)hipHostFree(slot.host);
    free_dev(slot.dev);
  }
  for (int i = 0; i < 4; ++i) {
    if (m->aux_stream[i] != nullptr) (void)hipStreamDestroy(m->aux_stream[i]);
    if (m->ev_join[i] != nullptr) (void)hipEventDestroy(m->ev_join[i]);
  }
  if (m->ev_fork != nullptr) (void)hipEventDestroy(m->ev_fork);
  if (m->d_kernels != nullptr) (void)hipFree(m->d_kernels);
  if (m->d_fft_mult != nullptr) (void)hipFree(m->d_fft_mult);
  if (m->d_fft_twiddle != nullptr) (void)hipFree(m->d_fft_twiddle);
  if (m->d_scratch64 != nullptr) (void)hipFree(m->d_scratch64);
  delete m;
  return DDD_OK;
}

int ddd_clear_forcing(ddd_model* m) {
  if (m != nullptr) { int rcj = chain_close(m); if (rcj) return rcj; }
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  free_dev(m->d_frc); free_dev(m->d_sp); free_dev(m->d_trig);
  if (m->d_runs != nullptr) (void)hipFree(m->d_runs);
  m->d_frc = nullptr; m->d_sp = nullptr; m->d_trig = nullptr; m->d_runs = nullptr;
  m->dp.trig = nullptr; m->dp.runs = nullptr;
  m->dp.forced = 0; m->dp.P = 0; m->dp.n_k = 0; m->dp.forcing_batch = 0;
  m->dp.inv_P = 0.0f; m->dp.inv_nk = 1.0f;
  m->dp.frc = nullptr; m->dp.sp = nullptr;
  return DDD_OK;
}

int ddd_set_forcing(ddd_model* m, int batch, int nparams, const float* amplitude,
                    const float* omega, const float* phase, const int32_t* k_index,
                    const float* spatial_phase, int n_k) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (m->spectral)
    return fail(DDD_ERR_UNSUPPORTED,
                "spectral models carry no forcing: apply finalize_time_derivative on the host");
  if (batch < 1 || nparams < 1 || n_k < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "batch, nparams and n_k must be >= 1");
  if (!amplitude || !omega || !phase || !k_index || !spatial_phase)
    return fail(DDD_ERR_INVALID_ARGUMENT, "NULL forcing table");
  int rc = ddd_clear_forcing(m);
  if (rc) return rc;
  if (!is_forced_family(m->cfg.equation)) return DDD_OK;   // finalize is the identity
  const size_t count = (size_t)batch * nparams;
  for (size_t i = 0; i < count; ++i)
    if (k_index[i] < 0 || k_index[i] >= n_k)
      return fail(DDD_ERR_INVALID_ARGUMENT, "k_index[%zu] = %d outside [0, %d)", i,
                  k_index[i], n_k);
  // Each sample's modes are stored sorted by k_index (stable), so that the
  // kernels sum the modes sharing a wavenumber over a contiguous range.
  std::vector<float4> packed(count);
  std::vector<int> order(nparams);
  for (int b = 0; b < batch; ++b) {
    const size_t base = (size_t)b * nparams;
    for (int j = 0; j < nparams; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
      return k_index[base + x] < k_index[base + y];
    });
    for (int j = 0; j < nparams; ++j) {
      const size_t i = base + order[j];
      float kbits;
      const int32_t ki = k_index[i];
      std::memcpy(&kbits, &ki, sizeof(kbits));
      packed[base + j] = make_float4(amplitude[i], omega[i], phase[i], kbits);
    }
  }
  std::vector<float> sp(spatial_phase, spatial_phase + (size_t)n_k * m->dp.N);
  // cos / sin of the (float32) spatial phase per grid point, [N][12] zero
  // padded (entry 2 k = cos, 2 k + 1 = sin of phase table row k; n_k <= 6)
  std::vector<float> trig((size_t)m->dp.N * 12, 0.0f);
  for (int x = 0; x < m->dp.N; ++x)
    for (int k = 0; k < n_k && k < 6; ++k) {
      const double theta = (double)sp[(size_t)k * m->dp.N + x];
      trig[(size_t)x * 12 + 2 * k + 0] = (float)std::cos(theta);
      trig[(size_t)x * 12 + 2 * k + 1] = (float)std::sin(theta);
    }
  // runs[b][kk] = first (sorted) mode of sample b whose k index is >= kk: the
  // kernels' per-(sample, k) sums cover modes [runs[kk], runs[kk + 1])
  std::vector<unsigned char> runs((size_t)batch * 8, 0);
  if (nparams < 256)
    for (int b = 0; b < batch; ++b) {
      int mode = 0;
      for (int kk = 0; kk < 8; ++kk) {
        while (mode < nparams) {
          int32_t ki;
          std::memcpy(&ki, &packed[(size_t)b * nparams + mode].w, sizeof(ki));
          if (ki >= kk) break;
          ++mode;
        }
        runs[(size_t)b * 8 + kk] = (unsigned char)mode;
      }
    }
  rc = upload(packed, &m->d_frc);
  if (!rc) rc = upload(sp, &m->d_sp);
  if (!rc) rc = upload(trig, &m->d_trig);
  if (!rc) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->d_runs), runs.size());
    if (e == hipSuccess)
      e = hipMemcpy(m->d_runs, runs.data(), runs.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(DDD_ERR_HIP, "forcing runs upload: %s", hipGetErrorString(e));
  }
  if (rc) return rc;
  m->dp.runs = m->d_runs;
  m->dp.trig = m->d_trig;
  m->dp.frc = m->d_frc;
  m->dp.sp = m->d_sp;
  m->dp.forced = 1;
  m->dp.P = nparams;
  m->dp.n_k = n_k;
  m->dp.inv_P = 1.0f / (float)nparams;
  m->dp.inv_nk = 1.0f / (float)std::max(n_k, 1);
  m->dp.forcing_batch = batch;
  return DDD_OK;
}

int ddd_time_derivative(ddd_model* m, double t, const float* y, float* dydt, int batch,
                        void* stream) {
  int rc = check_batch(m, batch);
  if (rc) return rc;
  if (batch > 0 && (!y || !dydt)) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  ddd::SubstepArgs a{};
  a.t = t; a.y_in = y; a.c1 = 1.0f; a.y_out = dydt; a.batch = batch;
  return substep_entry(m, a, static_cast<hipStream_t>(stream));
}

int ddd_rk_substep(ddd_model* m, double t, const float* y_in, const float* y_base,
                   float c1, float* y_out, const float* acc_in, float c2,
                   float* acc_out, int batch, void* stream) {
  int rc = check_batch(m, batch);
  if (rc) return rc;
  if (batch > 0 && !y_in) return fail(DDD_ERR_INVALID_ARGUMENT, "y_in is NULL");
  if (batch > 0 && !y_out && !acc_out)
    return fail(DDD_ERR_INVALID_ARGUMENT, "both y_out and acc_out are NULL");
  ddd::SubstepArgs a{};
  a.t = t; a.y_in = y_in; a.y_base = y_base; a.c1 = c1; a.y_out = y_out;
  a.acc_in = acc_in; a.c2 = c2; a.acc_out = acc_out; a.batch = batch;
  return substep_entry(m, a, static_cast<hipStream_t>(stream));
}

int ddd_stream_fork(ddd_model* m, void* stream) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (m->spectral)
    return fail(DDD_ERR_UNSUPPORTED, "spectral models have no chained substeps");
  int rc = chain_close(m);   // a region that is still open ends here
  if (rc) return rc;
  m->chain.open = true;
  m->chain.stream = static_cast<hipStream_t>(stream);
  return DDD_OK;
}

int ddd_set_region_mode(ddd_model* m, int mode) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (mode != DDD_REGION_AUTO && mode != DDD_REGION_CHAINS && mode != DDD_REGION_RING)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown region mode %d", mode);
  int rc = chain_close(m);
  if (rc) return rc;
  m->region_mode = mode;
  return DDD_OK;
}

int ddd_region_stats(const ddd_model* m, int64_t* ring_launches, int64_t* ring_commands) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  long long launches = 0, commands = 0;
  if (m->ring != nullptr) {
    std::lock_guard<std::mutex> lk(m->ring->mu);
    launches = (long long)m->ring->launches; commands = (long long)m->ring->commands;
  }
#ifdef DDD_RING_TRACE   // (variant build: where the stamps are)
  if (m->ring != nullptr) launches = (long long)(uintptr_t)(m->ring->status + 16);
#endif
  if (ring_launches != nullptr) *ring_launches = launches;
  if (ring_commands != nullptr) *ring_commands = commands;
  return DDD_OK;
}

int ddd_stream_join(ddd_model* m, void* stream) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (!m->chain.open) return DDD_OK;
  if (static_cast<hipStream_t>(stream) != m->chain.stream)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_stream_join: not the stream the region was opened on (ddd_stream_fork)");
  return chain_close(m);
}

int ddd_space_derivatives(ddd_model* m, const float* y, float* out, int batch,
                          void* stream) {
  if (m != nullptr) { int rcj = chain_close(m); if (rcj) return rcj; }
  int rc = check_batch(m, batch);
  if (rc) return rc;
  if (batch > 0 && (!y || !out)) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (!m->dp.fixed && m->dp.target != ddd::TARGET_COEFFICIENTS &&
      m->dp.target != ddd::TARGET_SPACE_DERIVATIVES)
    return fail(DDD_ERR_UNSUPPORTED, "model_target has no spatial derivatives");
  ddd::SubstepArgs a{};
  a.y_in = y; a.derivs_out = out; a.batch = batch;
  return launch_substep(m, plan_substep(m, a), a, static_cast<hipStream_t>(stream));
}

int ddd_coefficients(ddd_model* m, const float* y, float* out, int batch, void* stream) {
  if (m != nullptr) { int rcj = chain_close(m); if (rcj) return rcj; }
  int rc = check_batch(m, batch);
  if (rc) return rc;
  if (batch > 0 && (!y || !out)) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (!m->dp.fixed && m->dp.target != ddd::TARGET_COEFFICIENTS)
    return fail(DDD_ERR_UNSUPPORTED, "model_target does not produce coefficients");
  ddd::SubstepArgs a{};
  a.y_in = y; a.coeffs_out = out; a.batch = batch;
  return launch_substep(m, plan_substep(m, a), a, static_cast<hipStream_t>(stream));
}

int ddd_integrate_fixed(ddd_model* m, int scheme, int launch_mode, double t0, double dt,
                        int n_steps, int save_every, const float* y0, float* y_out,
                        int batch, void* stream_) {
  if (m != nullptr) { int rcj = chain_close(m); if (rcj) return rcj; }
  int rc = check_integrate_args(m, n_steps, save_every, y0, y_out, batch);
  if (rc) return rc;
  ddd::Tableau tab;
  rc = make_tableau(scheme, &tab);
  if (rc) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (launch_mode == DDD_LAUNCH_PERSISTENT) {
    ddd::IntegrateArgs a{};
    a.t0 = t0; a.dt = dt; a.n_steps = n_steps; a.save_every = save_every; a.tab = tab;
    a.sc = make_stage_consts(tab, dt);
    a.y0 = y0; a.y_out = y_out; a.batch = batch;
    return launch_integrate<float>(m, plan_launch(m, Op::persistent, {batch}), a, stream);
  }
  if (launch_mode != DDD_LAUNCH_PER_SUBSTEP && launch_mode != DDD_LAUNCH_PER_STEP)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown launch_mode %d", launch_mode);
  if (batch == 0 || n_steps == 0) return DDD_OK;

  // One fused launch per substep; the state lives in HBM between launches.
  const size_t elems = (size_t)batch * m->dp.N;
  rc = ensure_scratch(m, 3 * elems);
  if (rc) return rc;
  float* ping = m->d_scratch;
  float* pong = m->d_scratch + elems;
  float* ystage = m->d_scratch + 2 * elems;
  const float h = (float)dt;
  const ddd::StageConsts stage_consts = make_stage_consts(tab, dt);

  // large ensembles: two half-ensembles side by side (plan_slabs)
  const SlabPlan plan = plan_slabs(m, batch);
  const int halves = plan.halves;
  const int* half_batch = plan.half_batch;
  const int* slab_first = plan.slab_first;
  // DDD_LAUNCH_PER_STEP: a kernel that takes all stages of a step, if there is one
  Plan step_plan;
  if (launch_mode == DDD_LAUNCH_PER_STEP)
    step_plan = plan_launch(m, Op::step, {batch, false, false, false,
                                          aligned16(y0) && aligned16(y_out) && (elems % 4) == 0});
  if (step_plan.op == Op::step) m->last_plan = step_plan;
  if (step_plan.route == Route::stream_fixed) {
    // fixed stencils, all stages of a step in one launch of the streaming kernel: the
    // stage inputs stay in the block's LDS tile, 8 B per grid point and step;
    // persistent blocks (eight per CU) walk over the tiles
    const long pts = (long)(ddd::stream::kStepTile / m->dp.N) * m->dp.N;
    const int tiles = (int)(((long)elems + pts - 1) / pts);
    const int grid = std::min(tiles, 2 * device_simds());
    const float* y = y0;
    size_t snap = 0;
    for (int step = 0; step < n_steps; ++step) {
      const bool saving = (step + 1) % save_every == 0;
      float* ynew = saving ? y_out + snap * elems : (y == ping ? pong : ping);
      ddd::StepArgs sa{};
      sa.t = t0 + (double)step * dt; sa.dt = dt; sa.tab = tab; sa.sc = stage_consts;
      sa.y_in = y; sa.y_out = ynew; sa.batch = batch;
      ddd::stream::launch_fixed_step(dim3(grid), stream, m->dp, sa, tiles);
      y = ynew;
      if (saving) ++snap;
    }
    DDD_HIP(hipGetLastError());
    return DDD_OK;
  }
  hipStream_t lanes[kMaxParts] = {stream, stream, stream, stream};
  if (halves > 1) {
    rc = fork_lanes(m, stream, halves);
    if (rc) return rc;
    for (int i = 0; i < halves; ++i) lanes[i] = m->aux_stream[i];
  }
  size_t half_off[kMaxParts];
  for (int i = 0; i < kMaxParts; ++i) half_off[i] = (size_t)slab_first[i] * m->dp.N;
  const float* y = y0;
  size_t snap = 0;
#ifdef DDD_PROBES
  int walk_launch = 0;
#endif
  for (int step = 0; step < n_steps; ++step) {
    const double t = t0 + (double)step * dt;
    const bool saving = (step + 1) % save_every == 0;
    float* ynew = saving ? y_out + snap * elems : (y == ping ? pong : ping);
    if (step_plan.op == Op::step) {
      // all stages in one launch per half-ensemble (step_multi_kernel)
      for (int hf = 0; hf < halves; ++hf) {
        if (half_batch[hf] == 0) continue;
        const ddd::DevParams dp = launch_params(m, step_plan, slab_first[hf]);
        ddd::StepArgs sa{};
        sa.t = t; sa.dt = dt; sa.tab = tab; sa.sc = stage_consts;
        sa.y_in = y + half_off[hf]; sa.y_out = ynew + half_off[hf]; sa.batch = half_batch[hf];
        const int groups = group_count(m, step_plan.geo, half_batch[hf]);
        const int grid = std::min(groups, resident_groups(step_plan.geo) / halves);
        with_equation(step_plan.eq, [&](auto eq) {
          constexpr int EQ = decltype(eq)::value;
          if (step_plan.tile == Tile::half)
            ddd::launch::step_half_spec<EQ>(dp, sa, groups, grid, lanes[hf]);
          else
            ddd::launch::step_spec<EQ>(step_plan.geo.rows, dp, sa, groups, grid, lanes[hf]);
        });
      }
      if (hipGetLastError() != hipSuccess) {
        rc = fail(DDD_ERR_HIP, "step launch failed");
        break;
      }
      y = ynew;
      if (saving) ++snap;
      continue;
    }
    const float* acc = nullptr;   // nullptr: accumulator still equals y
    for (int s = 0; s < tab.stages; ++s) {
      const bool last = s == tab.stages - 1;
      const bool accumulate = tab.b[s] != 0.0f || last;
      for (int hf = 0; hf < halves; ++hf) {
        const size_t off = half_off[hf];
        ddd::SubstepArgs a{};
        a.t = t + tab.c[s] * dt;
        a.y_in = (s == 0 ? y : ystage) + off;
        a.batch = half_batch[hf];
        if (!last) {   // next stage input  y + a_{s+1} h f
          a.y_base = y + off; a.c1 = tab.a[s + 1] * h; a.y_out = ystage + off;
        }
        if (accumulate) {
          a.acc_in = (acc != nullptr ? acc : y) + off;
          a.c2 = tab.b[s] * h;
          a.acc_out = ynew + off;
        }
#ifdef DDD_PROBES
        a.trace = reinterpret_cast<unsigned long long*>(g_debug.walk_trace_ptr);
        a.trace_row0 = walk_launch++ * ddd::kWalkTraceRows;
#endif
        rc = launch_substep(m, plan_substep(m, a), a, lanes[hf], slab_first[hf], halves);
        if (rc) break;
      }
      if (rc) break;
      if (accumulate) acc = ynew;
    }
    if (rc) break;   // (the join below still runs: the internal streams may be busy)
    y = ynew;
    if (saving) ++snap;
  }
  if (halves > 1) {
    const int rc_join = join_lanes(m, stream, halves);
    if (rc == DDD_OK) rc = rc_join;
  }
  return rc;
}

int ddd_integrate_fixed_f64(ddd_model* m, int scheme, double t0, double dt, int n_steps,
                            int save_every, const double* y0, double* y_out, int batch,
                            void* stream) {
  if (m != nullptr) { int rcj = chain_close(m); if (rcj) return rcj; }
  if (m != nullptr && m->spectral) {
    // float64 state AND right-hand side, one fused launch per substep
    if (batch < 0 || n_steps < 0 || save_every < 1)
      return fail(DDD_ERR_INVALID_ARGUMENT, "bad batch / n_steps / save_every");
    if (batch == 0 || n_steps == 0) return DDD_OK;
    if (y0 == nullptr || y_out == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
    ddd::Tableau tab;
    int rcs = make_tableau(scheme, &tab);
    if (rcs) return rcs;
    double b64[ddd::kMaxStages];
    tableau_weights_f64(scheme, b64);
    const size_t elems = (size_t)batch * m->sp.N;
    if (m->scratch64_doubles < 3 * elems) {
      if (m->d_scratch64 != nullptr) (void)hipFree(m->d_scratch64);
      m->d_scratch64 = nullptr; m->scratch64_doubles = 0;
      DDD_HIP(hipMalloc(reinterpret_cast<void**>(&m->d_scratch64), 3 * elems * sizeof(double)));
      m->scratch64_doubles = 3 * elems;
    }
    double* ping = m->d_scratch64;
    double* pong = ping + elems;
    double* ystage = ping + 2 * elems;
    const double* y = y0;
    size_t snap = 0;
    for (int step = 0; step < n_steps; ++step) {
      const bool saving = (step + 1) % save_every == 0;
      double* ynew = saving ? y_out + snap * elems : (y == ping ? pong : ping);
      const double* acc = nullptr;
      for (int s = 0; s < tab.stages; ++s) {
        ddd::spectral::SubstepArgs64 a{};
        a.y_in = s == 0 ? y : ystage;
        a.batch = batch;
        const bool last = s == tab.stages - 1;
        if (!last) { a.y_base = y; a.c1 = (double)tab.a[s + 1] * dt; a.y_out = ystage; }
        if (tab.b[s] != 0.0f || last) {
          a.acc_in = acc != nullptr ? acc : y;
          a.c2 = b64[s] * dt;
          a.acc_out = ynew;
          acc = ynew;
        }
        rcs = launch_spectral(m, a, static_cast<hipStream_t>(stream));
        if (rcs) return rcs;
      }
      y = ynew;
      if (saving) ++snap;
    }
    return DDD_OK;
  }
  int rc = check_integrate_args(m, n_steps, save_every, y0, y_out, batch);
  if (rc) return rc;
  ddd::IntegrateArgs a{};
  rc = make_tableau(scheme, &a.tab);
  if (rc) return rc;
  a.t0 = t0; a.dt = dt; a.n_steps = n_steps; a.save_every = save_every;
  a.sc = make_stage_consts(a.tab, dt);
  a.y0 = y0; a.y_out = y_out; a.batch = batch;
  return launch_integrate<double>(m, plan_launch(m, Op::persistent, {batch, true}), a,
                                  static_cast<hipStream_t>(stream));
}

namespace {

// Argument checks of the adaptive entry points (solo and population).
int check_adaptive_args(const ddd_model* m, const double* times, int n_times, double rtol,
                        double atol, double max_step, const double* y0, const double* y_out,
                        const int32_t* nfev, const int32_t* status, int batch) {
  int rc = check_batch(m, batch, m->spectral);
  if (rc) return rc;
  if (times == nullptr || n_times < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "times must hold at least one value");
  if (n_times >= (1 << 28))   // (the packed per-sample controllers keep the output index in 28 bits)
    return fail(DDD_ERR_INVALID_ARGUMENT, "n_times = %d: at most 2^28 - 1 output times", n_times);
  for (int i = 0; i < n_times; ++i)
    if (!std::isfinite(times[i]) || (i > 0 && !(times[i] > times[i - 1])))
      return fail(DDD_ERR_INVALID_ARGUMENT, "times must be finite and strictly increasing");
  if (!(rtol > 0.0) || !(atol >= 0.0) || !(max_step > 0.0))
    return fail(DDD_ERR_INVALID_ARGUMENT, "rtol and max_step must be positive, atol >= 0");
  if (batch > 0 && (!y0 || !y_out || !nfev || !status))
    return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  return DDD_OK;
}

// The output times of one adaptive call, on their way to the device through the next slot of
// the model's page-locked ring (ddd_model::TimeSlot); *out: the slot, whose `dev` the launch
// reads and whose `done` event the caller records again behind that launch.
int stage_times(ddd_model* m, const double* times, int n_times, hipStream_t stream,
                ddd_model::TimeSlot** out) {
  // the caller's array may be gone before the copy runs: upload from a page-locked
  // copy the model owns until the launch that reads it has finished
  ddd_model::TimeSlot& slot = m->time_slot[m->next_time_slot];
  m->next_time_slot = (m->next_time_slot + 1) % ddd_model::kTimeSlots;
  if (slot.in_flight) {   // only when kTimeSlots adaptive calls are still queued
    DDD_HIP(hipEventSynchronize(slot.done));
    slot.in_flight = false;
  }
  if (slot.capacity < (size_t)n_times) {
    if (slot.host != nullptr) (void)hipHostFree(slot.host);
    free_dev(slot.dev);
    slot.host = nullptr; slot.dev = nullptr; slot.capacity = 0;
    DDD_HIP(hipHostMalloc(reinterpret_cast<void**>(&slot.host), (size_t)n_times * sizeof(double),
                          hipHostMallocDefault));
    DDD_HIP(hipMalloc(reinterpret_cast<void**>(&slot.dev), (size_t)n_times * sizeof(double)));
    slot.capacity = (size_t)n_times;
  }
  if (slot.done == nullptr)
    DDD_HIP(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
  std::memcpy(slot.host, times, (size_t)n_times * sizeof(double));
  DDD_HIP(hipMemcpyAsync(slot.dev, slot.host, (size_t)n_times * sizeof(double),
                         hipMemcpyHostToDevice, stream));
  // the slot is busy from HERE on (the copy reads the pinned buffer), whatever happens to
  // the launch that follows: an error return between the copy and the launch must not leave a
  // slot that looks free while the copy is still pending
  DDD_HIP(hipEventRecord(slot.done, stream));
  slot.in_flight = true;
  *out = &slot;
  return DDD_OK;
}

// max_attempts <= 0: a thousand times the attempts of a run at max_step
long long attempt_limit(const double* times, int n_times, double max_step, long long max_attempts) {
  if (max_attempts > 0) return max_attempts;
  const double span = times[n_times - 1] - times[0];
  return (long long)std::min(1e15, std::ceil(span / max_step) * 1000.0 + 100000.0);
}

}  // namespace

int ddd_integrate_adaptive_f64(ddd_model* m, const double* times, int n_times, double rtol,
                               double atol, double max_step, long long max_attempts,
                               const double* y0, double* y_out, int32_t* nfev,
                               int32_t* status, int batch, void* stream_) {
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  int rc = chain_close(m);
  if (rc) return rc;
  rc = check_adaptive_args(m, times, n_times, rtol, atol, max_step, y0, y_out, nfev, status, batch);
  if (rc) return rc;
  if (m->spectral && is_forced_family(m->cfg.equation))
    return fail(DDD_ERR_UNSUPPORTED,
                "the spectral adaptive kernel carries no forcing term: Burgers' forcing(t) "
                "(equations.py:276-277) would be dropped; integrate it with the host driver "
                "(integrate.odeint over ddd_time_derivative_f64 + finalize_time_derivative)");
  if (batch == 0) return DDD_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ddd_model::TimeSlot* slot_ptr = nullptr;
  rc = stage_times(m, times, n_times, stream, &slot_ptr);
  if (rc) return rc;
  ddd_model::TimeSlot& slot = *slot_ptr;
  ddd::AdaptiveArgs a{};
  // ... and is free again once the launch enqueued below has run
  const auto enqueued = [&]() -> int {
    DDD_HIP(hipGetLastError());
    DDD_HIP(hipEventRecord(slot.done, stream));
    slot.in_flight = true;
    return DDD_OK;
  };
  a.times = slot.dev; a.n_times = n_times;
  a.rtol = rtol; a.atol = atol; a.max_step = max_step;
  a.y0 = y0; a.y_out = y_out; a.nfev = nfev; a.status = status; a.batch = batch;
  a.max_attempts = attempt_limit(times, n_times, max_step, max_attempts);
  const Plan p = plan_launch(m, Op::adaptive, {batch, true});
  m->last_plan = p;
  if (p.route == Route::spectral) {
    // float64 right-hand side (SpectralDifferentiator), one workgroup per sample
    const size_t lds = ddd::spectral::lds_bytes(m->sp);
    const int pts = (m->sp.N + ddd::spectral::kThreads - 1) / ddd::spectral::kThreads;
#define DDD_SPECTRAL_ADAPTIVE(PTS)                                                           \
    do {                                                                                     \
      DDD_HIP(hipFuncSetAttribute(                                                           \
          reinterpret_cast<const void*>(ddd::spectral::adaptive_kernel<PTS>),                \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                            \
      hipLaunchKernelGGL((ddd::spectral::adaptive_kernel<PTS>), dim3(batch),                 \
                         dim3(ddd::spectral::kThreads), lds, stream, m->sp, a);              \
    } while (0)
    if (pts <= 1) DDD_SPECTRAL_ADAPTIVE(1);
    else if (pts <= 2) DDD_SPECTRAL_ADAPTIVE(2);
    else if (pts <= 4) DDD_SPECTRAL_ADAPTIVE(4);
    else DDD_SPECTRAL_ADAPTIVE(8);
#undef DDD_SPECTRAL_ADAPTIVE
    return enqueued();
  }
  if (p.route == Route::weno) {
    // the WENO5 + Godunov-flux exact solver: one wavefront and one controller per sample
    ddd::launch::weno_adaptive(m->dp, a, stream);
    return enqueued();
  }
  if (p.route == Route::generic) {
    // generic right-hand side (nets the MFMA path does not carry, WENO on grids that are
    // not 64 x {1, 2, 4, 8} points): one workgroup and one controller per sample
    const size_t lds = ddd::generic::adaptive_lds_bytes(m->dp);
    if (lds > 160 * 1024)
      return fail(DDD_ERR_UNSUPPORTED,
                  "generic adaptive kernel needs %zu B of LDS per sample (limit 163840)", lds);
    DDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ddd::generic::adaptive_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ddd::generic::adaptive_kernel, dim3(batch), dim3(ddd::generic::kThreads),
                       lds, stream, m->dp, a);
    return enqueued();
  }
  const ddd::DevParams dp = launch_params(m, p);
  const int blocks = group_count(m, p.geo, batch);
  if (p.eq >= 0) {
    with_equation(p.eq, [&](auto eq) {
      constexpr int EQ = decltype(eq)::value;
      if (p.tile == Tile::quad) ddd::launch::adaptive_quad_spec<EQ>(dp, a, blocks, stream);
      else if (p.tile == Tile::half) ddd::launch::adaptive_half_spec<EQ>(dp, a, blocks, stream);
      else ddd::launch::adaptive_spec<EQ>(p.geo.rows, dp, a, blocks, stream);
    });
  } else if (m->big()) {
    with_big_tower(m, p.geo.rows, [&](auto k, auto cb, auto rows) {
      ddd::launch::adaptive_big_unit<decltype(k)::value, decltype(cb)::value, decltype(rows)::value>(
          dp, a, blocks, stream);
    });
  } else {
    with_rows(p.geo.rows, [&](auto rows) {
      if (m->wide) ddd::launch::adaptive_wide_unit<decltype(rows)::value>(dp, a, blocks, stream);
      else ddd::launch::adaptive_runtime_unit<decltype(rows)::value>(dp, a, blocks, stream);
    });
  }
  return enqueued();
}

// ---- replica populations in one launch (mfma_population.hip) ---------------------------
struct ddd_population {
  ddd_model* model0 = nullptr;   // everything that is not a weight, at call time (launch_params)
  int replicas = 0;
  float* d_w_input = nullptr;    // [R][stride]: the replicas' packed weights, copied at creation
  float* d_w_hidden = nullptr;
  float* d_w_final4 = nullptr;
  ddd::PopulationStrides strides{};   // (the weight strides; the output strides are per call)
  ddd::packdev::Tables tables{};      // what ddd_population_load_weights packs by (model0's)
  size_t n_weights = 0;               // floats of a replica's natural-layout weight vector
};

namespace {

// Equation, grid, tower, head and scaling of two configurations are the same.  Of
// derivative_orders[] and input_sizes[] only the num_derivatives entries in use are compared
// (a C caller may leave the rest unset); reserved[] is not looked at.
bool same_architecture(const ddd_config& a, const ddd_config& b) {
  if (a.equation != b.equation || a.num_points != b.num_points ||
      a.num_derivatives != b.num_derivatives || a.dx != b.dx || a.period != b.period ||
      a.eta != b.eta || a.standard_deviation != b.standard_deviation ||
      a.stencil_size != b.stencil_size || a.model_target != b.model_target ||
      a.num_layers != b.num_layers || a.filter_size != b.filter_size ||
      a.kernel_size != b.kernel_size || a.activation != b.activation ||
      a.polynomial_accuracy_order != b.polynomial_accuracy_order ||
      a.ensure_unbiased_coefficients != b.ensure_unbiased_coefficients ||
      a.weno_reconstruction != b.weno_reconstruction)
    return false;
  for (int d = 0; d < a.num_derivatives && d < DDD_MAX_DERIVATIVES; ++d)
    if (a.derivative_orders[d] != b.derivative_orders[d] || a.input_sizes[d] != b.input_sizes[d])
      return false;
  return true;
}

// The plan of a population launch on model m, or DDD_ERR_UNSUPPORTED with the reason.
int plan_population(const ddd_model* m, Op op, int batch, Plan* out, const char* who) {
  CallFacts f{batch, op == Op::adaptive};
  f.population = true;
  *out = plan_launch(m, op, f);
  if (out->no_population != nullptr)
    return fail(DDD_ERR_UNSUPPORTED, "%s: no population kernel for this configuration: %s%s%s",
                who, out->no_population,
                out->route != Route::mfma && !m->mfma_reason.empty() ? ": " : "",
                out->route != Route::mfma ? m->mfma_reason.c_str() : "");
  return DDD_OK;
}

// replica r's weights in place of model 0's
ddd::DevParams population_params(ddd_population* pop, const Plan& p) {
  ddd::DevParams dp = launch_params(pop->model0, p);
  dp.w_input = pop->d_w_input;
  dp.w_hidden = pop->d_w_hidden;
  dp.w_final4 = pop->d_w_final4;
  return dp;
}

}  // namespace

int ddd_population_destroy(ddd_population* pop) {
  if (pop == nullptr) return DDD_OK;
  free_dev(pop->d_w_input); free_dev(pop->d_w_hidden); free_dev(pop->d_w_final4);
  delete pop;
  return DDD_OK;
}

namespace {

// What a population asks of each of its models: a population form of both integrators
// (whatever forcing the model carries now: the call plans again) and the three packed arrays.
int check_population_model(const ddd_model* m, const char* who) {
  Plan p;
  int rc = plan_population(m, Op::adaptive, 1, &p, who);
  if (!rc) rc = plan_population(m, Op::persistent, 1, &p, who);
  if (rc) return rc;
  if (m->d_w_input == nullptr || m->d_w_hidden == nullptr || m->d_w_final4 == nullptr ||
      m->n_w_input != (size_t)ddd::packdev::kInputFloats ||
      m->n_w_hidden != (size_t)ddd::packdev::kHiddenFloats ||
      m->n_w_final4 != (size_t)ddd::packdev::kFinal4Floats)
    return fail(DDD_ERR_UNSUPPORTED, "%s: packed weight arrays of other sizes than the "
                "population kernels read", who);
  return DDD_OK;
}

// The handle around model0 with room for `replicas` sets of packed weights (not yet filled).
int new_population(ddd_model* m0, int replicas, ddd_population** out) {
  ddd_population* pop = new ddd_population();
  pop->model0 = m0;
  pop->replicas = replicas;
  pop->strides.w_input = (long long)m0->n_w_input;
  pop->strides.w_hidden = (long long)m0->n_w_hidden;
  pop->strides.w_final4 = (long long)m0->n_w_final4;
  // ddd_population_load_weights: the tables of pack_device.h, model0's
  const ddd::DevParams& dp = m0->dp;
  ddd::packdev::Tables& t = pop->tables;
  std::memcpy(t.ns8, dp.ns8, sizeof(t.ns8));
  std::memcpy(t.bias8, dp.bias8, sizeof(t.bias8));
  for (int d = 0; d < ddd::packdev::kDerivs; ++d) {
    t.in_start[d] = dp.in_start[d];
    t.in_size[d] = dp.in_size[d];
  }
  for (int l = 0; l < ddd::packdev::kLayers; ++l) { t.w_off[l] = dp.w_off[l]; t.b_off[l] = dp.b_off[l]; }
  t.K = dp.K; t.F = dp.F; t.C_out = dp.C_out; t.D = dp.D; t.G = dp.G;
  t.fin4_groups = dp.fin4_groups;
  t.spec_folded = m0->spec_folded ? 1 : 0;
  pop->n_weights = (size_t)dp.b_off[dp.L - 1] + (size_t)dp.cout[dp.L - 1];
  const auto room = [&](float** dst, size_t n) -> int {
    DDD_HIP(hipMalloc(reinterpret_cast<void**>(dst), (size_t)replicas * n * sizeof(float)));
    return DDD_OK;
  };
  int rc = room(&pop->d_w_input, m0->n_w_input);
  if (!rc) rc = room(&pop->d_w_hidden, m0->n_w_hidden);
  if (!rc) rc = room(&pop->d_w_final4, m0->n_w_final4);
  if (rc) { ddd_population_destroy(pop); return rc; }
  *out = pop;
  return DDD_OK;
}

// Replica r's three arrays = model m's, device to device (the caller synchronises).
int copy_packed(ddd_population* pop, int r, const ddd_model* m) {
  const auto copy = [&](float* dst, size_t n, const float* src) -> int {
    DDD_HIP(hipMemcpy(dst + (size_t)r * n, src, n * sizeof(float), hipMemcpyDeviceToDevice));
    return DDD_OK;
  };
  int rc = copy(pop->d_w_input, m->n_w_input, m->d_w_input);
  if (!rc) rc = copy(pop->d_w_hidden, m->n_w_hidden, m->d_w_hidden);
  if (!rc) rc = copy(pop->d_w_final4, m->n_w_final4, m->d_w_final4);
  return rc;
}

}  // namespace

int ddd_population_create(ddd_model* const* models, int replicas, ddd_population** out) {
  if (out == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (models == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "models is NULL");
  if (replicas < 1 || replicas > DDD_MAX_REPLICAS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "replicas = %d outside [1, %d]", replicas,
                DDD_MAX_REPLICAS);
  for (int r = 0; r < replicas; ++r) {
    if (models[r] == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "models[%d] is NULL", r);
    for (int q = 0; q < r; ++q)
      if (models[q] == models[r])
        return fail(DDD_ERR_INVALID_ARGUMENT, "models[%d] and models[%d] are the same model", q, r);
  }
  const ddd_model* m0 = models[0];
  for (int r = 1; r < replicas; ++r) {
    const ddd_model* m = models[r];
    if (!same_architecture(m->cfg, m0->cfg))
      return fail(DDD_ERR_UNSUPPORTED,
                  "models[%d]: ddd_config differs from models[0]'s (replicas share one "
                  "architecture: equation, grid, tower, head, standard deviation)", r);
  }
  for (int r = 0; r < replicas; ++r) {
    const ddd_model* m = models[r];
    char who[32];
    snprintf(who, sizeof(who), "models[%d]", r);
    int rc = check_population_model(m, who);
    if (rc) return rc;
    const ddd::DevParams& a = m->dp;
    const ddd::DevParams& b = m0->dp;
    if (std::memcmp(a.ns8, b.ns8, sizeof(a.ns8)) != 0 ||
        std::memcmp(a.bias8, b.bias8, sizeof(a.bias8)) != 0 || a.dsel_bits != b.dsel_bits ||
        a.dsel_valid != b.dsel_valid || m->spec_folded != m0->spec_folded ||
        a.fin4_groups != b.fin4_groups || a.exact_div != b.exact_div)
      return fail(DDD_ERR_UNSUPPORTED,
                  "models[%d]: projection tables differ from models[0]'s (the replicas' "
                  "launch reads models[0]'s)", r);
  }
  ddd_population* pop = nullptr;
  int rc = new_population(models[0], replicas, &pop);
  if (rc) return rc;
  for (int r = 0; r < replicas && !rc; ++r) rc = copy_packed(pop, r, models[r]);
  if (!rc) DDD_HIP(hipDeviceSynchronize());   // (the copies have read the models' arrays)
  if (rc) { ddd_population_destroy(pop); return rc; }
  *out = pop;
  return DDD_OK;
}

int ddd_population_create_replicated(ddd_model* model, int replicas, ddd_population** out) {
  if (out == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (model == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (replicas < 1 || replicas > DDD_MAX_REPLICAS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "replicas = %d outside [1, %d]", replicas,
                DDD_MAX_REPLICAS);
  int rc = check_population_model(model, "model");
  if (rc) return rc;
  ddd_population* pop = nullptr;
  rc = new_population(model, replicas, &pop);
  if (rc) return rc;
  for (int r = 0; r < replicas && !rc; ++r) rc = copy_packed(pop, r, model);
  if (!rc) DDD_HIP(hipDeviceSynchronize());
  if (rc) { ddd_population_destroy(pop); return rc; }
  *out = pop;
  return DDD_OK;
}

int ddd_population_load_weights(ddd_population* pop, const float* weights, size_t n_weights,
                                int first_replica, int count, void* stream) {
  if (pop == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "population is NULL");
  if (weights == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "weights is NULL");
  if (first_replica < 0 || count < 0)
    return fail(DDD_ERR_INVALID_ARGUMENT, "first_replica = %d, count = %d: negative",
                first_replica, count);
  if (n_weights == 0) return fail(DDD_ERR_INVALID_ARGUMENT, "n_weights = 0");
  if (count > pop->replicas - first_replica)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "replicas %d .. %d outside the population's 0 .. %d", first_replica,
                first_replica + count - 1, pop->replicas - 1);
  if (n_weights != pop->n_weights)
    return fail(DDD_ERR_INVALID_ARGUMENT, "n_weights = %zu, the model has %zu floats",
                n_weights, pop->n_weights);
  if (count == 0) return DDD_OK;
  ddd::packdev::launch_pack(
      pop->tables, weights, (long long)n_weights,
      pop->d_w_input + (size_t)first_replica * ddd::packdev::kInputFloats,
      pop->d_w_hidden + (size_t)first_replica * ddd::packdev::kHiddenFloats,
      pop->d_w_final4 + (size_t)first_replica * ddd::packdev::kFinal4Floats, count,
      static_cast<hipStream_t>(stream));
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_population_integrate_adaptive_f64(ddd_population* pop, const double* times, int n_times,
                                          double rtol, double atol, double max_step,
                                          long long max_attempts, const double* y0,
                                          double* y_out, int32_t* nfev, int32_t* status,
                                          int batch, void* stream_) {
  if (pop == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "population is NULL");
  ddd_model* m = pop->model0;
  int rc = chain_close(m);
  if (rc) return rc;
  rc = check_adaptive_args(m, times, n_times, rtol, atol, max_step, y0, y_out, nfev, status, batch);
  if (rc) return rc;
  if (batch == 0) return DDD_OK;
  Plan p;
  rc = plan_population(m, Op::adaptive, batch, &p, "models[0]");
  if (rc) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ddd_model::TimeSlot* slot = nullptr;
  rc = stage_times(m, times, n_times, stream, &slot);
  if (rc) return rc;
  ddd::AdaptiveArgs a{};
  a.times = slot->dev; a.n_times = n_times;
  a.rtol = rtol; a.atol = atol; a.max_step = max_step;
  a.y0 = y0; a.y_out = y_out; a.nfev = nfev; a.status = status; a.batch = batch;
  a.max_attempts = attempt_limit(times, n_times, max_step, max_attempts);
  m->last_plan = p;
  const ddd::DevParams dp = population_params(pop, p);
  ddd::PopulationStrides s = pop->strides;
  s.y_out = (long long)n_times * batch * m->dp.N;
  s.samples = batch;
  const int groups = group_count(m, p.geo, batch);
  with_equation(p.eq, [&](auto eq) {
    ddd::launch::adaptive_population_spec<decltype(eq)::value>(dp, a, s, groups, pop->replicas,
                                                               stream);
  });
  DDD_HIP(hipGetLastError());
  DDD_HIP(hipEventRecord(slot->done, stream));   // the slot is free once the launch has run
  slot->in_flight = true;
  return DDD_OK;
}

int ddd_population_integrate_fixed(ddd_population* pop, int scheme, double t0, double dt,
                                   int n_steps, int save_every, const float* y0, float* y_out,
                                   int batch, void* stream_) {
  if (pop == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "population is NULL");
  ddd_model* m = pop->model0;
  int rc = chain_close(m);
  if (rc) return rc;
  rc = check_integrate_args(m, n_steps, save_every, y0, y_out, batch);
  if (rc) return rc;
  ddd::IntegrateArgs a{};
  rc = make_tableau(scheme, &a.tab);
  if (rc) return rc;
  if (batch == 0 || n_steps == 0) return DDD_OK;
  Plan p;
  rc = plan_population(m, Op::persistent, batch, &p, "models[0]");
  if (rc) return rc;
  a.t0 = t0; a.dt = dt; a.n_steps = n_steps; a.save_every = save_every;
  a.sc = make_stage_consts(a.tab, dt);
  a.y0 = y0; a.y_out = y_out; a.batch = batch;
  m->last_plan = p;
  const ddd::DevParams dp = population_params(pop, p);
  ddd::PopulationStrides s = pop->strides;
  s.y_out = (long long)(n_steps / save_every) * batch * m->dp.N;
  s.samples = batch;
  const int groups = group_count(m, p.geo, batch);
  with_equation(p.eq, [&](auto eq) {
    ddd::launch::integrate_population_spec<decltype(eq)::value>(
        dp, a, s, groups, pop->replicas, static_cast<hipStream_t>(stream_));
  });
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_circulant_apply_f64(const double* kernel, const double* in, double* out, int rows,
                            int n, void* stream) {
  if (!kernel || !in || !out) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (rows < 0 || n < 1 || n > ddd::spectral::kMaxPoints)
    return fail(DDD_ERR_INVALID_ARGUMENT, "rows >= 0 and 1 <= n <= %d required",
                ddd::spectral::kMaxPoints);
  if (rows == 0) return DDD_OK;
  const size_t lds = 2 * (size_t)n * sizeof(double);
  hipLaunchKernelGGL(ddd::spectral::circulant_apply_kernel, dim3(rows),
                     dim3(ddd::spectral::kThreads), lds, static_cast<hipStream_t>(stream),
                     kernel, in, out, n);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_conv1d_periodic(const float* in, const float* filters, const float* bias,
                        float* out, int batch, int n, int cin, int cout, int k,
                        int center, int activation, void* stream) {
  if (!in || !filters || !out) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (batch < 0 || n < 1 || cin < 1 || cout < 1 || k < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "bad conv1d shape");
  if (activation < -1 || activation > DDD_ACT_ELU)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown activation %d", activation);
  const long total = (long)batch * n * cout;
  if (total == 0) return DDD_OK;
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(ddd::ops::conv1d_periodic_kernel, dim3(blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, filters, bias, out, batch, n,
                     cin, cout, k, center ? k / 2 : 0, activation);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_pad_periodic(const float* in, float* out, int batch, int n, int c, int padding,
                     int center, void* stream) {
  if (!in || !out) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (batch < 0 || n < 1 || c < 1 || padding < 0)
    return fail(DDD_ERR_INVALID_ARGUMENT, "bad pad_periodic shape");
  const long total = (long)batch * (n + padding) * c;
  if (total == 0) return DDD_OK;
  const int left = center ? (padding + 1) / 2 : 0;   // layers.py:76-79
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(ddd::ops::pad_periodic_kernel, dim3(blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, out, batch, n, c, padding, left);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_extract_patches(const float* in, float* out, int batch, int n, int size, void* stream) {
  if (!in || !out) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (batch < 0 || n < 1 || size < 1) return fail(DDD_ERR_INVALID_ARGUMENT, "bad sizes");
  if (batch == 0) return DDD_OK;
  const long total = (long)batch * n * size;
  const int blocks = (int)std::min<long>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(ddd::ops::extract_patches_kernel, dim3(blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, out, batch, n, size);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_apply_coefficients(const float* coefficients, const float* in, float* out, int batch,
                           int n, int d, int g, void* stream) {
  if (!coefficients || !in || !out) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (batch < 0 || n < 1 || d < 1 || g < 1) return fail(DDD_ERR_INVALID_ARGUMENT, "bad sizes");
  if (batch == 0) return DDD_OK;
  const long total = (long)batch * n * d;
  const int blocks = (int)std::min<long>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(ddd::ops::apply_coefficients_kernel, dim3(blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), coefficients, in, out, batch, n, d, g);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_apply_space_derivatives(int equation, const float* derivatives, const float* y,
                                float* out, int batch, int n, int d, double eta, double dx,
                                void* stream) {
  if (!derivatives || !y || !out) return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (equation < DDD_EQ_BURGERS || equation > DDD_EQ_KS_GODUNOV)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown equation %d", equation);
  if (batch < 0 || n < 2 || d < 1 || d > DDD_MAX_DERIVATIVES || !(dx > 0))
    return fail(DDD_ERR_INVALID_ARGUMENT, "bad sizes");
  if (batch == 0) return DDD_OK;
  const bool flux_form = equation == DDD_EQ_BURGERS_CONSERVATIVE ||
                         equation == DDD_EQ_KDV_CONSERVATIVE ||
                         equation == DDD_EQ_KS_CONSERVATIVE || equation >= DDD_EQ_BURGERS_GODUNOV;
  const size_t lds = (size_t)n * sizeof(float);
  if (lds > 64 * 1024) return fail(DDD_ERR_UNSUPPORTED, "num_points too large");
  hipLaunchKernelGGL(ddd::ops::apply_space_derivatives_kernel, dim3(batch), dim3(256), lds,
                     static_cast<hipStream_t>(stream), derivatives, y, out, equation, n, d,
                     (float)eta, (float)(1.0 / dx), flux_form ? 1 : 0);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

int ddd_polynomial_accuracy_apply(const float* inputs, const float* nullspace,
                                  const float* bias, float* out, int64_t m,
                                  int input_size, int g, void* stream) {
  if (!inputs || !nullspace || !bias || !out)
    return fail(DDD_ERR_INVALID_ARGUMENT, "NULL array");
  if (m < 0 || input_size < 1 || g < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "bad polynomial_accuracy shape");
  if (m == 0) return DDD_OK;
  const long total = (long)m * g;
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(ddd::ops::polynomial_accuracy_kernel, dim3(blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), inputs, nullspace, bias, out,
                     (long)m, input_size, g);
  DDD_HIP(hipGetLastError());
  return DDD_OK;
}

static_assert(ddd::rollout::kMaxQuantiles == DDD_ROLLOUT_MAX_QUANTILES &&
                  ddd::rollout::kMaxStopTimes == DDD_ROLLOUT_MAX_STOP_TIMES &&
                  ddd::rollout::kMaxPoints == DDD_ROLLOUT_MAX_POINTS &&
                  ddd::rollout::kMaxFactor == DDD_ROLLOUT_MAX_FACTOR,
              "rollout_scores.h / ddd1d.h");

int ddd_rollout_reference(const ddd_rollout_reference_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_rollout_reference_args);
  if (a->num_samples < 1 || a->num_times < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_samples = %d, num_times = %d (both >= 1)",
                a->num_samples, a->num_times);
  if (a->num_points < 1 || a->num_points > DDD_ROLLOUT_MAX_POINTS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_points = %d out of range [1, %d]", a->num_points,
                DDD_ROLLOUT_MAX_POINTS);
  if (a->num_points_exact < a->num_points || a->num_points_exact % a->num_points != 0)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "num_points_exact = %d is not a multiple of num_points = %d",
                a->num_points_exact, a->num_points);
  const int factor = a->num_points_exact / a->num_points;
  if (factor > DDD_ROLLOUT_MAX_FACTOR)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "num_points_exact / num_points = %d out of range [1, %d]", factor,
                DDD_ROLLOUT_MAX_FACTOR);
  if (!a->y_exact || !a->exact_low)
    return fail(DDD_ERR_INVALID_ARGUMENT, "y_exact and exact_low must not be NULL");
  const size_t outputs = (size_t)a->num_samples * a->num_times * a->num_points;
  if ((outputs + ddd::rollout::kThreads - 1) / ddd::rollout::kThreads > 0x7fffffffu)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "num_samples num_times num_points = %zu: too many for one launch", outputs);
  ddd::rollout::ReferenceParams p;
  p.y_exact = a->y_exact;
  p.exact_low = a->exact_low;
  p.S = a->num_samples;
  p.T = a->num_times;
  p.N = a->num_points;
  p.f = factor;
  DDD_HIP(ddd::rollout::launch_reference(p, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

namespace {

int rollout_sizes(int replicas, int num_times, int num_samples, int num_quantiles) {
  if (replicas < 1 || replicas > DDD_MAX_REPLICAS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "replicas = %d out of range [1, %d]", replicas,
                DDD_MAX_REPLICAS);
  if (num_times < 1 || num_samples < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_times = %d, num_samples = %d (both >= 1)",
                num_times, num_samples);
  if (num_quantiles < 1 || num_quantiles > DDD_ROLLOUT_MAX_QUANTILES)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_quantiles = %d out of range [1, %d]",
                num_quantiles, DDD_ROLLOUT_MAX_QUANTILES);
  // (one group of lanes per row, at least four rows per workgroup)
  if ((size_t)replicas * num_times * num_samples > 0x7fffffffu)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "replicas num_times num_samples = %zu: too many rows for one launch",
                (size_t)replicas * num_times * num_samples);
  return DDD_OK;
}

}  // namespace

size_t ddd_rollout_scores_workspace_bytes(int replicas, int num_times, int num_samples,
                                          int num_quantiles) {
  if (rollout_sizes(replicas, num_times, num_samples, num_quantiles)) return 0;
  return ddd::rollout::workspace_bytes(replicas, num_times, num_samples, num_quantiles);
}

int ddd_rollout_scores(const ddd_rollout_scores_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_rollout_scores_args);
  int rc = rollout_sizes(a->replicas, a->num_times, a->num_samples, a->num_quantiles);
  if (rc) return rc;
  if (a->num_points < 1 || a->num_points > DDD_ROLLOUT_MAX_POINTS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_points = %d out of range [1, %d]", a->num_points,
                DDD_ROLLOUT_MAX_POINTS);
  if (a->num_stop_times < 1 || a->num_stop_times > DDD_ROLLOUT_MAX_STOP_TIMES)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_stop_times = %d out of range [1, %d]",
                a->num_stop_times, DDD_ROLLOUT_MAX_STOP_TIMES);
  if (a->dtype != DDD_ROLLOUT_F64 && a->dtype != DDD_ROLLOUT_F32)
    return fail(DDD_ERR_INVALID_ARGUMENT, "dtype = %d (DDD_ROLLOUT_F64 or DDD_ROLLOUT_F32)",
                a->dtype);
  if (!a->y_model || !a->exact_low || !a->mae || !a->survival)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "y_model, exact_low, mae and survival must not be NULL");
  if (!a->times || !a->max_error || !a->frac_good || !a->stop_times)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "times, max_error, frac_good and stop_times must not be NULL");
  for (int t = 0; t < a->num_times; ++t)
    if (!std::isfinite(a->times[t]) || (t > 0 && !(a->times[t] > a->times[t - 1])))
      return fail(DDD_ERR_INVALID_ARGUMENT, "times must be finite and strictly increasing");
  const size_t ws = ddd::rollout::workspace_bytes(a->replicas, a->num_times, a->num_samples,
                                                  a->num_quantiles);
  if (a->workspace == nullptr || a->workspace_bytes < ws)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "workspace of %zu bytes given, ddd_rollout_scores_workspace_bytes = %zu",
                a->workspace == nullptr ? (size_t)0 : a->workspace_bytes, ws);
  ddd::rollout::ScoreParams p;
  std::memset(&p, 0, sizeof(p));
  p.y_model = a->y_model;
  p.exact_low = a->exact_low;
  p.f32 = a->dtype == DDD_ROLLOUT_F32;
  p.R = a->replicas;
  p.T = a->num_times;
  p.S = a->num_samples;
  p.N = a->num_points;
  p.Q = a->num_quantiles;
  p.K = a->num_stop_times;
  for (int q = 0; q < p.Q; ++q) {
    p.max_error[q] = a->max_error[q];
    p.frac_good[q] = a->frac_good[q];
  }
  for (int k = 0; k < p.K; ++k) {   // (the times increase: the rows kept are a prefix)
    int kept = 0;
    while (kept < p.T && a->times[kept] <= a->stop_times[k]) ++kept;
    p.kept[k] = kept;
  }
  char* base = static_cast<char*>(a->workspace);
  p.row_abs_sum = a->row_abs_sum != nullptr ? a->row_abs_sum : reinterpret_cast<double*>(base);
  base += ddd::rollout::row_sum_bytes(p.R, p.T, p.S);
  p.good = a->good != nullptr ? a->good : reinterpret_cast<uint8_t*>(base);
  base += ddd::rollout::good_bytes(p.R, p.T, p.S, p.Q);
  p.times = reinterpret_cast<double*>(base);
  p.mae = a->mae;
  p.survival = a->survival;
  DDD_HIP(ddd::rollout::launch_scores(p, a->times, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

int ddd_set_kernel(ddd_model* m, int kind) {
  if (m != nullptr) { int rcj = chain_close(m); if (rcj) return rcj; }
  if (m == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "model is NULL");
  if (m->spectral) return fail(DDD_ERR_UNSUPPORTED, "spectral models have one kernel");
  switch (kind) {
    case DDD_KERNEL_AUTO:
      m->kernel = m->mfma_ok ? DDD_KERNEL_MFMA : DDD_KERNEL_GENERIC;
      m->force_rows = 0;
      m->explicit_kernel = false;
      m->last_plan = Plan{};
      return DDD_OK;
    case DDD_KERNEL_GENERIC:
      m->kernel = DDD_KERNEL_GENERIC;
      m->explicit_kernel = true;
      m->last_plan = Plan{};
      return DDD_OK;
    case DDD_KERNEL_MFMA:
    case DDD_KERNEL_MFMA_ROWS64:
    case DDD_KERNEL_MFMA_ROWS256:
    case DDD_KERNEL_MFMA_ROWS64_W32:
    case DDD_KERNEL_MFMA_ROWS64_W16:
      if (!m->mfma_ok)
        return fail(DDD_ERR_UNSUPPORTED, "MFMA path unavailable for this model: %s",
                    m->mfma_reason.c_str());
      if (kind == DDD_KERNEL_MFMA_ROWS64_W32 && (m->wide || m->big()))
        return fail(DDD_ERR_UNSUPPORTED,
                    "the two-wave split exists for the 5-tap x 32-filter tower with stencils <= 8 "
                    "points / <= 16 channels only");
      if (kind == DDD_KERNEL_MFMA_ROWS64_W16 && m->dp.w_quad == nullptr)
        return fail(DDD_ERR_UNSUPPORTED,
                    "four 16-row wavefronts per group exist for three-layer 5-tap x 32-filter nets "
                    "with <= 16 output channels only");
      if ((kind == DDD_KERNEL_MFMA_ROWS64 || kind == DDD_KERNEL_MFMA_ROWS64_W32 ||
           kind == DDD_KERNEL_MFMA_ROWS64_W16) &&
          !(m->dp.N <= 64 && 64 % m->dp.N == 0))
        return fail(DDD_ERR_UNSUPPORTED,
                    "64-row workgroups need num_points to divide 64 (got %d)", m->dp.N);
      m->kernel = DDD_KERNEL_MFMA;
      m->explicit_kernel = true;
      m->force_rows = kind == DDD_KERNEL_MFMA_ROWS64 ? 64
                      : kind == DDD_KERNEL_MFMA_ROWS64_W32 ? 32
                      : kind == DDD_KERNEL_MFMA_ROWS64_W16 ? 16
                      : kind == DDD_KERNEL_MFMA_ROWS256 ? 256 : 0;
      m->last_plan = Plan{};
      return DDD_OK;
    default:
      return fail(DDD_ERR_INVALID_ARGUMENT, "unknown kernel kind %d", kind);
  }
}

// The name of the plan the most recent launch ran.  With no launch recorded (a fresh
// handle, or ddd_set_kernel since the last launch): spectral, then WENO, then generic, then
// the MFMA name of the geometry alone (mfma_geometry: r256, r64w32 or r64).
const char* ddd_kernel_name(const ddd_model* m) {
  if (m == nullptr) return "";
  if (m->last_plan.name != nullptr) return m->last_plan.name;
  Plan p;
  p.route = m->spectral ? Route::spectral
            : use_weno_kernel(m) ? Route::weno
            : m->kernel != DDD_KERNEL_MFMA ? Route::generic : Route::mfma;
  if (p.route == Route::mfma) {
    p.geo = mfma_geometry(m);
    if (p.geo.wave_rows == 32) p.tile = Tile::split;
  }
  return plan_name(p);
}

int64_t ddd_fma_per_point(const ddd_model* m) { return m ? m->fma_per_point : 0; }

#ifdef DDD_PROBES
// Profiling / A-B switches (not part of the product API; every change is
// logged).  Names: no_fold (takes effect at ddd_model_create), no_spec,
// no_stream, prio_split, stagger, substep_parts, ablate, trace_ptr, walk_trace_ptr; "reset" puts
// every switch back to its default (the switches are process-global).
DDD_API int ddd_debug_set_option(const char* name, long long value) {
  if (name == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "name is NULL");
  const std::string key(name);
  if (key == "no_fold") g_debug.no_fold = (int)value;
  else if (key == "no_spec") g_debug.no_spec = (int)value;
  else if (key == "no_stream") g_debug.no_stream = (int)value;
  else if (key == "no_lean") g_debug.no_lean = (int)value;
  else if (key == "no_weno") g_debug.no_weno = (int)value;
  else if (key == "no_fft") g_debug.no_fft = (int)value;
  else if (key == "no_half") g_debug.no_half = (int)value;
  else if (key == "prio_split") g_debug.prio_split = (int)value;
  else if (key == "stagger") g_debug.stagger = (int)value;
  else if (key == "substep_parts") g_debug.substep_parts = (int)value;
  else if (key == "reset") g_debug = DebugOptions{};   // every switch back to its default
  else if (key == "ablate") g_debug.ablate = (int)value;
  else if (key == "trace_ptr") g_debug.trace_ptr = (unsigned long long)value;
  else if (key == "walk_trace_ptr") g_debug.walk_trace_ptr = (unsigned long long)value;
  else return fail(DDD_ERR_INVALID_ARGUMENT, "unknown debug option '%s'", name);
  fprintf(stderr, "libddd1d: debug option %s = %lld%s\n", name, value,
          key == "ablate" && value != 0 ? " (kernel phases skipped: results are WRONG)" : "");
  return DDD_OK;
}

DDD_API int ddd_debug_hwid(unsigned* out_host, int blocks, int spin) {
  unsigned* d = nullptr;
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d), (size_t)blocks * 4 * sizeof(unsigned)));
  hipLaunchKernelGGL(ddd::ops::hwid_probe_kernel, dim3(blocks), dim3(64), 0, nullptr, d, spin);
  DDD_HIP(hipGetLastError());
  DDD_HIP(hipMemcpy(out_host, d, (size_t)blocks * 4 * sizeof(unsigned), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return DDD_OK;
}

// Issue-port sharing probe (ops.h: issue_share_probe_kernel).  Returns mean
// s_memtime ticks per operation for the MFMA streamers (slot 0) and the
// workers (slot 1) over `blocks` workgroups.
DDD_API int ddd_debug_issue_share(int mfma_kind, int work_kind, int blocks, int iters, int prio,
                          double* mfma_ticks_per_op, double* work_ticks_per_op) {
  unsigned long long* d = nullptr;
  const size_t words = (size_t)blocks * 8 * 4;
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d), words * sizeof(unsigned long long)));
  DDD_HIP(hipMemset(d, 0, words * sizeof(unsigned long long)));
#define DDD_SHARE(M, W)                                                                  \
  if (mfma_kind == M && work_kind == W)                                                  \
    hipLaunchKernelGGL((ddd::ops::issue_share_probe_kernel<M, W>), dim3(blocks), dim3(512), \
                       0, nullptr, d, iters, 1.0f, prio);
  for (int rep = 0; rep < 2; ++rep) {
    DDD_SHARE(0, 1) DDD_SHARE(0, 2) DDD_SHARE(0, 3) DDD_SHARE(0, 4)
    DDD_SHARE(1, 0) DDD_SHARE(1, 1) DDD_SHARE(1, 2) DDD_SHARE(1, 3) DDD_SHARE(1, 4)
    DDD_SHARE(2, 0) DDD_SHARE(2, 1) DDD_SHARE(2, 2) DDD_SHARE(2, 3) DDD_SHARE(2, 4)
    DDD_SHARE(3, 0) DDD_SHARE(3, 1) DDD_SHARE(3, 2) DDD_SHARE(4, 0) DDD_SHARE(4, 1) DDD_SHARE(4, 2)
    DDD_SHARE(5, 0) DDD_SHARE(5, 1) DDD_SHARE(5, 2) DDD_SHARE(5, 3) DDD_SHARE(6, 0) DDD_SHARE(6, 1) DDD_SHARE(6, 2)
    DDD_SHARE(7, 0) DDD_SHARE(7, 1) DDD_SHARE(7, 2) DDD_SHARE(8, 0) DDD_SHARE(8, 1) DDD_SHARE(8, 2) DDD_SHARE(8, 3)
    DDD_HIP(hipDeviceSynchronize());
  }
#undef DDD_SHARE
  DDD_HIP(hipGetLastError());
  std::vector<unsigned long long> h(words);
  DDD_HIP(hipMemcpy(h.data(), d, words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  double sm = 0, sw = 0;
  long nm = 0, nw = 0;
  for (size_t g = 0; g < (size_t)blocks * 8; ++g) {
    const unsigned slot = (unsigned)(h[g * 4 + 1] & 0xff);
    if (slot == 0) { sm += (double)h[g * 4]; ++nm; } else { sw += (double)h[g * 4]; ++nw; }
  }
  const double mops = (double)iters * ((mfma_kind == 2 || mfma_kind >= 7) ? 256.0 : 64.0);
  const double wops = (double)iters * 64.0;
  *mfma_ticks_per_op = nm ? sm / nm / mops : 0.0;
  *work_ticks_per_op = nw ? sw / nw / wops : 0.0;
  return DDD_OK;
}

DDD_API int ddd_debug_mfma_rate(int chains, int is32, int blocks, int iters, double* ticks_per_mfma,
                        double* wall_ns_per_mfma) {
  unsigned long long* d = nullptr;
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d), (size_t)blocks * 2 * sizeof(unsigned long long)));
  hipEvent_t e0, e1;
  DDD_HIP(hipEventCreate(&e0));
  DDD_HIP(hipEventCreate(&e1));
  for (int rep = 0; rep < 2; ++rep) {
    DDD_HIP(hipEventRecord(e0, nullptr));
#define DDD_RATE(C, W) hipLaunchKernelGGL((ddd::ops::mfma_rate_probe_kernel<C, W>), dim3(blocks), dim3(64), 0, nullptr, d, iters, 1.0f)
#define DDD_RATE4(C) hipLaunchKernelGGL((ddd::ops::mfma4_rate_probe_kernel<C>), dim3(blocks), dim3(64), 0, nullptr, d, iters, 1.0f)
    if (is32 == 2) {   // v_mfma_f32_4x4x1_16b_f32, 24 per iteration
      if (chains == 1) DDD_RATE4(1); else if (chains == 2) DDD_RATE4(2);
      else if (chains == 3) DDD_RATE4(3); else DDD_RATE4(4);
    } else if (is32) { if (chains == 1) DDD_RATE(1, true); else if (chains == 2) DDD_RATE(2, true); else DDD_RATE(4, true); }
    else { if (chains == 1) DDD_RATE(1, false); else if (chains == 2) DDD_RATE(2, false); else DDD_RATE(4, false); }
#undef DDD_RATE4
#undef DDD_RATE
    DDD_HIP(hipEventRecord(e1, nullptr));
    DDD_HIP(hipEventSynchronize(e1));
  }
  float ms = 0.0f;
  DDD_HIP(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> h((size_t)blocks * 2);
  DDD_HIP(hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  double sum = 0.0;
  for (int b = 0; b < blocks; ++b) sum += (double)h[(size_t)b * 2];
  const double per_iter = is32 == 2 ? 24.0 : 8.0;
  *ticks_per_mfma = sum / blocks / ((double)iters * per_iter);
  *wall_ns_per_mfma = (double)ms * 1e6 / ((double)iters * per_iter);
  return DDD_OK;
}
#endif  // DDD_PROBES

int ddd_selftest_mfma_layout(void) {
  float* d32 = nullptr;
  float* d16 = nullptr;
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d32), 32 * 32 * sizeof(float)));
  DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d16), 16 * 16 * sizeof(float)));
  hipLaunchKernelGGL(ddd::ops::mfma_layout_probe_kernel, dim3(1), dim3(64), 0, nullptr,
                     d32, d16);
  DDD_HIP(hipGetLastError());
  std::vector<float> h32(32 * 32), h16(16 * 16);
  DDD_HIP(hipMemcpy(h32.data(), d32, h32.size() * sizeof(float), hipMemcpyDeviceToHost));
  DDD_HIP(hipMemcpy(h16.data(), d16, h16.size() * sizeof(float), hipMemcpyDeviceToHost));
  (void)hipFree(d32);
  (void)hipFree(d16);
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      const float want = (float)(i + 1) * (float)(64 * (j + 1)) +
                         (float)(1000 + i) * (float)(3 * j + 7);
      if (h32[i * 32 + j] != want)
        return fail(DDD_ERR_UNSUPPORTED,
                    "mfma_f32_32x32x2 layout mismatch at D[%d][%d]: got %g want %g", i, j,
                    h32[i * 32 + j], want);
    }
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      float want = 0.0f;
      for (int k = 0; k < 4; ++k)
        want = fmaf((float)((k + 1) * 100 + i), (float)((k + 2) * (j + 1)), want);
      if (h16[i * 16 + j] != want)
        return fail(DDD_ERR_UNSUPPORTED,
                    "mfma_f32_16x16x4 layout mismatch at D[%d][%d]: got %g want %g", i, j,
                    h16[i * 16 + j], want);
    }
  {
    // 4x4x1 (16 blocks) with the A block broadcast: register r of lane l must be
    // A(lane 4 abid + r) * B(lane l) + C   (ops.h: mfma4_bcast)
    float* d4 = nullptr;
    DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d4), 16 * 4 * 64 * sizeof(float)));
    hipLaunchKernelGGL(ddd::ops::mfma4_layout_probe_kernel, dim3(1), dim3(64), 0, nullptr, d4);
    DDD_HIP(hipGetLastError());
    std::vector<float> h4(16 * 4 * 64);
    DDD_HIP(hipMemcpy(h4.data(), d4, h4.size() * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(d4);
    for (int abid = 0; abid < 16; ++abid)
      for (int r = 0; r < 4; ++r)
        for (int l = 0; l < 64; ++l) {
          const float want = fmaf((float)(1000 * abid + r + 1), (float)(l + 1), 0.5f);
          const float got = h4[(abid * 4 + r) * 64 + l];
          if (got != want)
            return fail(DDD_ERR_UNSUPPORTED,
                        "mfma_f32_4x4x1 broadcast layout mismatch at abid %d reg %d lane %d: "
                        "got %g want %g", abid, r, l, got, want);
        }
  }
  {
    // relu as the [0, 1] output clamp of a packed add on activations scaled by
    // 2^-kReluShift (rhs_mfma.h: activate16), and the constant-lane-mask select of the
    // input layer (upper_half_one)
    std::vector<float> h_in(128);
    const float dn = std::ldexp(1.0f, -ddd::kReluShift);
    for (int i = 0; i < 128; ++i) {
      const float mag = std::ldexp(1.0f + 0.0078125f * (float)i, (i * 7) % 120 - 60);   // 2^-60 .. 2^59
      h_in[i] = ((i % 3) == 1 ? -mag : mag) * dn;
    }
    h_in[5] = 0.0f; h_in[6] = -0.0f; h_in[7] = std::nanf(""); h_in[8] = 2.0f;   // (> 1: saturates)
    h_in[9] = -INFINITY; h_in[10] = INFINITY; h_in[11] = 1.0f;
    float *d_in = nullptr, *d_out = nullptr;
    DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d_in), 128 * sizeof(float)));
    DDD_HIP(hipMalloc(reinterpret_cast<void**>(&d_out), 192 * sizeof(float)));
    DDD_HIP(hipMemcpy(d_in, h_in.data(), 128 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ddd::ops::relu_clamp_probe_kernel, dim3(1), dim3(64), 0, nullptr, d_in, d_out);
    DDD_HIP(hipGetLastError());
    std::vector<float> h_out(192);
    DDD_HIP(hipMemcpy(h_out.data(), d_out, 192 * sizeof(float), hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < 2; ++e) {
        const float x = h_in[2 * l + e], got = h_out[64 * e + l];
        const float want = std::isnan(x) ? 0.0f : x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x;
        if (!(got == want) || std::signbit(got))
          return fail(DDD_ERR_UNSUPPORTED,
                      "v_pk_add_f32 ... clamp is not the [0, 1] clamp the relu assumes: "
                      "input %g (element %d of pair %d) gave %g, want %g", x, e, l, got, want);
      }
    for (int l = 0; l < 64; ++l)
      if (h_out[128 + l] != (l < 32 ? (float)l : 1.0f))
        return fail(DDD_ERR_UNSUPPORTED, "constant-lane-mask select: lane %d gave %g", l,
                    h_out[128 + l]);
  }
  // informational: the kernels fall back to ds_bpermute when this is 0
  (void)dpp_wave_rol_ok();
  return DDD_OK;
}

}  // extern "C"
