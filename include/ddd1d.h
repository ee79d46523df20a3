/*
 * ddd1d.h -- C ABI of libddd1d.so, the MI355X (gfx950) implementation of the
 * per-timestep learned-stencil integration path of
 * google/data-driven-discretization-1d (package pde_superresolution).
 *
 * The reference has no FFI: its plug-in seam for this path is the Python
 * callable `Differentiator.__call__(t, y) -> dy/dt` (integrate.py:40-45)
 * consumed by `integrate.odeint` (integrate.py:143-169), plus the batched
 * fixed-step `model.integrate_ode` (model.py:138-159).  Each entry point below
 * names the reference interface it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Every function returns 0 on success and a negative ddd_status on error;
 *     ddd_last_error() returns a thread-local human readable message.  No C++
 *     exception crosses this boundary.
 *   - `ddd_model*` is an opaque handle owned by the caller until
 *     ddd_model_destroy().  One handle per host thread / GPU; calls on one
 *     handle are stream ordered and must not be issued concurrently.
 *   - Unless marked HOST, pointers are device pointers (HBM) valid on the
 *     current HIP device.  `stream` is a hipStream_t passed as void* (NULL =
 *     the default stream).  Nothing here synchronises the device except
 *     ddd_model_create / ddd_set_forcing (which copy small host tables).
 *   - Batches are row major [batch][x] ("batch-major"): one sample's N grid
 *     points are contiguous, so a wavefront's 64 lanes read 256 contiguous
 *     bytes.  All data arithmetic is IEEE float32 (the reference's TF graph
 *     dtype); the `_f64` entry points keep the *integration state* in float64
 *     like SciPy does on the reference's host side.
 */
#ifndef DDD1D_H_
#define DDD1D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDD_ABI_VERSION 1
/* libddd1d.so is built with -fvisibility=hidden: the entry points below are its
 * whole dynamic symbol table (tests/test_cpu_host_api.py compares `nm -D`
 * with this header). */
#if defined(__GNUC__)
#define DDD_API __attribute__((visibility("default")))
#else
#define DDD_API
#endif
#define DDD_MAX_DERIVATIVES 4 /* Godunov KS uses 4 (equations.py:570-574) */
#define DDD_MAX_STENCIL 16
#define DDD_MAX_LAYERS 8
#define DDD_MAX_STAGES 4

typedef enum ddd_status {
  DDD_OK = 0,
  DDD_ERR_INVALID_ARGUMENT = -1,
  DDD_ERR_UNSUPPORTED = -2,
  DDD_ERR_HIP = -3,
  DDD_ERR_NO_DEVICE = -4
} ddd_status;

/* equations.py: EQUATION_TYPES / CONSERVATIVE_EQUATION_TYPES / FLUX_EQUATION_TYPES
 * (:590-606).  Derivative order of the entries of `derivative_orders` must be
 * the class's DERIVATIVE_ORDERS. */
typedef enum ddd_equation {
  DDD_EQ_BURGERS = 0,              /* equations.py:230-302  (u_x, u_xx)        */
  DDD_EQ_BURGERS_CONSERVATIVE = 1, /* equations.py:323-338  (u, u_x)           */
  DDD_EQ_KDV = 2,                  /* equations.py:373-439  (u_x, u_xxx)       */
  DDD_EQ_KDV_CONSERVATIVE = 3,     /* equations.py:442-457  (u, u_xx)          */
  DDD_EQ_KS = 4,                   /* equations.py:481-548  (u_x, u_xx, u_xxxx)*/
  DDD_EQ_KS_CONSERVATIVE = 5,      /* equations.py:551-567  (u, u_x, u_xxx)    */
  DDD_EQ_BURGERS_GODUNOV = 6,      /* equations.py:352-370  (u-, u+, u_x)      */
  DDD_EQ_KDV_GODUNOV = 7,          /* equations.py:460-478  (u-, u+, u_xx)     */
  DDD_EQ_KS_GODUNOV = 8            /* equations.py:570-587  (u-, u+, u_x, u_xxx)*/
} ddd_equation;

/* model.py:411-417 (_NONLINEARITIES) */
typedef enum ddd_activation {
  DDD_ACT_RELU = 0,
  DDD_ACT_RELU6 = 1,
  DDD_ACT_TANH = 2,
  DDD_ACT_SOFTPLUS = 3,
  DDD_ACT_ELU = 4
} ddd_activation;

/* hparams.model_target, model.py:579-640 */
typedef enum ddd_model_target {
  DDD_TARGET_COEFFICIENTS = 0,
  DDD_TARGET_SPACE_DERIVATIVES = 1,
  DDD_TARGET_TIME_DERIVATIVE = 2,
  DDD_TARGET_FLUX = 3
} ddd_model_target;

/* Fixed-step explicit Runge-Kutta schemes.  MIDPOINT is
 * tf.contrib.integrate.odeint_fixed(method='midpoint') as called from
 * model.integrate_ode (model.py:155-157); BS3 is the Bogacki-Shampine tableau
 * of SciPy's RK23 (the reference's production integrator, integrate.py:154)
 * without step-size control. */
typedef enum ddd_scheme {
  DDD_SCHEME_EULER = 0,
  DDD_SCHEME_MIDPOINT = 1,
  DDD_SCHEME_BS3 = 2,
  DDD_SCHEME_RK4 = 3
} ddd_scheme;

typedef enum ddd_kernel_kind {
  DDD_KERNEL_AUTO = 0,    /* MFMA path when the configuration allows it */
  DDD_KERNEL_GENERIC = 1, /* any configuration, scalar FMA, one block / sample */
  DDD_KERNEL_MFMA = 2,    /* f32 MFMA tiles; 64 or 256 grid points / block    */
  DDD_KERNEL_MFMA_ROWS64 = 3,  /* force one-wavefront workgroups (N divides 64) */
  DDD_KERNEL_MFMA_ROWS256 = 4, /* force four-wavefront workgroups               */
  DDD_KERNEL_MFMA_ROWS64_W32 = 5, /* force 64-row groups on two 32-row wavefronts */
  DDD_KERNEL_MFMA_ROWS64_W16 = 6  /* force 64-row groups on FOUR 16-row wavefronts
                                     (small ensembles: one sample on the four SIMDs of
                                     a CU; per-equation float32 integrators only)      */
} ddd_kernel_kind;

/* How ddd_integrate_fixed advances time. */
typedef enum ddd_launch_mode {
  DDD_LAUNCH_PERSISTENT = 0, /* time loop inside ONE launch, state in registers */
  DDD_LAUNCH_PER_SUBSTEP = 1, /* one fused launch per RK substep, state in HBM  */
  DDD_LAUNCH_PER_STEP = 2 /* all stages of a step in one launch, state through HBM
                           * once per step (models on a per-equation MFMA kernel;
                           * others advance substep by substep)                */
} ddd_launch_mode;

/* Static description of one model: the equation (equations.py), the solution
 * grid (equations.py:44-68) and the conv-net hyper-parameters
 * (training.py:127-141). */
typedef struct ddd_config {
  int32_t struct_size; /* = sizeof(ddd_config), checked */
  int32_t equation;    /* ddd_equation */
  int32_t num_points;  /* N = grid.solution_num_points */
  int32_t num_derivatives;
  int32_t derivative_orders[DDD_MAX_DERIVATIVES];
  double dx;                 /* grid.solution_dx */
  double period;             /* grid.period */
  double eta;                /* Burgers viscosity, else 0 */
  double standard_deviation; /* Equation.standard_deviation (input scaling) */
  int32_t stencil_size;      /* G: 7 centered / 6 staggered by default */
  int32_t model_target;      /* ddd_model_target */
  int32_t num_layers;        /* conv layers incl. the linear output layer */
  int32_t filter_size;       /* hidden channels (32) */
  int32_t kernel_size;       /* conv taps (5) */
  int32_t activation;        /* ddd_activation */
  int32_t polynomial_accuracy_order;    /* 0: net emits D*G coefficients */
  int32_t ensure_unbiased_coefficients; /* only with accuracy order 0 */
  int32_t input_sizes[DDD_MAX_DERIVATIVES]; /* null-space dims per derivative */
  int32_t weno_reconstruction; /* ddd_baseline_create only: 1 = derivative slots
                                * 0 and 1 (u_minus, u_plus of the Godunov
                                * equations) are WENO5 reconstructions
                                * (weno.py:43-123, integrate.py:124-140,
                                * model.py:82-88) instead of stencil rows */
  int32_t reserved[3];
} ddd_config;

typedef struct ddd_model ddd_model;

/* ---- lifecycle ---------------------------------------------------------- */

/* Replaces: SavedModelDifferentiator.__init__ (integrate.py:51-68), i.e.
 * building model.predict_time_derivative (model.py:618-640) and restoring the
 * checkpoint.  HOST inputs:
 *   weights   layer-major; per layer the conv kernel [K][Cin][Cout] (the
 *             tf.layers.conv1d variable layout) followed by the bias [Cout].
 *             Cin = 1 for the first layer, filter_size otherwise; Cout =
 *             filter_size for hidden layers and, for the output layer,
 *             sum(input_sizes) (coefficients target, accuracy order > 0),
 *             D*G (accuracy order 0), D (space_derivatives) or 1.
 *   nullspace per derivative [input_size][G], float32 of
 *             PolynomialAccuracyLayer.nullspace (polynomials.py:246-264);
 *             NULL unless target = coefficients with accuracy order > 0.
 *   bias      [D][G] float32 of PolynomialAccuracyLayer.bias; same condition.
 * Which kernel family serves the model (ddd_kernel_name; training.py:127-141 leaves
 * these hyper-parameters free): 8 <= num_points <= 256, >= 2 layers, kernel_size <= 7 and
 * filter_size <= 64 (not both > 5 and > 32): the f32-MFMA kernels -- 5 taps x 32 filters with
 * per-equation kernels, 7 x 32 / 5 x 64 / 3 x 32 with streamed weights, nets in between
 * embedded exactly with zero weights; num_layers = 1 with coefficient output: affine
 * coefficients folded here, evaluated by the lane == grid point kernel (persistent
 * launches, num_points | 64, float32 state: "valu_f32_lean") or on the VALU route of the
 * MFMA-path kernels; everything else (larger nets or grids, num_points < 8, stencils > 12
 * points): the generic kernel.
 */
DDD_API int ddd_model_create(const ddd_config* cfg, const float* weights,
                     size_t n_weights, const float* nullspace,
                     size_t n_nullspace, const float* bias, size_t n_bias,
                     ddd_model** out);

/* Replaces: PolynomialDifferentiator.__init__ (integrate.py:77-103) /
 * model.baseline_space_derivatives (model.py:59-112): fixed stencils.
 * HOST `stencils` is [D][G] float32, each derivative's standard coefficients
 * (polynomials.coefficients) centred in a common G-wide window so that tap i
 * multiplies u[x + i - G/2] (the alignment of layers.pad_periodic(center=True),
 * layers.py:76-79).  Net fields of cfg are ignored.  Also used for
 * num_layers = 0 models (model.py:496-502) after folding on the host. */
DDD_API int ddd_baseline_create(const ddd_config* cfg, const float* stencils,
                        size_t n_stencils, ddd_model** out);

/* Replaces: integrate.SpectralDifferentiator.__init__ (integrate.py:110-111)
 * and the ExactMethod.SPECTRAL branch of model.baseline_space_derivatives
 * (model.py:78-80): the fine-grid "exact" solver of KdV / KS.  Float64.
 * HOST `kernels` is [D][N] float64: for each derivative the response of the
 * reference's spectral operator to a unit impulse at x = 0
 * (scipy.fftpack.diff(delta, order, period) for SpectralDifferentiator,
 * duckarray.spectral_derivative(delta, order, period) for the TF-graph form),
 * so that deriv[x] = sum_j kernels[d][(x - j) mod N] * y[j].
 * Non-flux equations only (DDD_EQ_BURGERS, DDD_EQ_KDV, DDD_EQ_KS:
 * integrate.py:346-347), N <= 2048.  Only the *_f64 entry points below accept
 * such a model; it carries no forcing (finalize_time_derivative stays on the
 * host, where the reference evaluates it in float64).
 * num_points a power of two >= 512: the same operators run as an in-LDS float64 FFT
 * (multipliers = the DFT of `kernels`, formed here in extended precision, so the
 * conventions of the call that produced the kernels carry over); smaller grids: the
 * O(N^2) circulant products. */
DDD_API int ddd_spectral_create(const ddd_config* cfg, const double* kernels,
                        size_t n_kernels, ddd_model** out);

DDD_API int ddd_model_destroy(ddd_model* model);

/* ---- per-sample forcing -------------------------------------------------
 * Replaces: RandomForcing.__call__ inside finalize_time_derivative
 * (equations.py:214-219, 276-277), one parameter row per sample.  HOST inputs,
 * all [batch][nparams]:
 *   amplitude  a_j            (times the exact block-mean factor when the grid
 *                              resamples by 'mean', i.e. conservative equations)
 *   omega      omega_j
 *   phase      phi_j          (plus the block-centre shift for 'mean')
 *   k_index    row of `spatial_phase` to use for mode j
 *   spatial_phase [n_k][N]    float32(2 pi k x_i / period) for each distinct k
 * forcing_b(x_i, t) = sum_j amplitude * sin((omega*t + spatial_phase) + phase),
 * accumulated in float32 in that order (the TF graph's order).  Ignored by
 * equations whose finalize_time_derivative is the identity (KdV, KS). */
DDD_API int ddd_set_forcing(ddd_model* model, int batch, int nparams,
                    const float* amplitude, const float* omega,
                    const float* phase, const int32_t* k_index,
                    const float* spatial_phase, int n_k);
DDD_API int ddd_clear_forcing(ddd_model* model);

/* ---- the hot path --------------------------------------------------------*/

/* Replaces: Differentiator.__call__(t, y) (integrate.py:70-71, 94-95), batched:
 * dydt[b] = finalize_time_derivative(t, predict_time_derivative(y[b])).
 * y, dydt: [batch][N] float32. */
DDD_API int ddd_time_derivative(ddd_model* model, double t, const float* y,
                        float* dydt, int batch, void* stream);

/* ONE fused launch = one Runge-Kutta substep:
 *     f       = time_derivative(t, y_in)
 *     y_out   = y_base + c1 * f          (y_base NULL -> c1 * f)
 *     acc_out = acc_in + c2 * f          (skipped when acc_out NULL;
 *                                         acc_in NULL -> c2 * f)
 * All arrays [batch][N] float32; y_out / acc_out may alias their inputs. */
DDD_API int ddd_rk_substep(ddd_model* model, double t, const float* y_in,
                   const float* y_base, float c1, float* y_out,
                   const float* acc_in, float c2, float* acc_out, int batch,
                   void* stream);

/* A caller that owns the Runge-Kutta loop -- the shape of integrate.odeint
 * (integrate.py:143-169: the driver calls the right-hand side once per stage) --
 * gets the library's own per-substep throughput by bracketing its loop:
 *
 *     ddd_stream_fork(model, stream);
 *     for (...) { ddd_rk_substep(model, ..., stream); ddd_rk_substep(model, ..., stream); }
 *     ddd_stream_join(model, stream);
 *
 * Inside the region, ddd_rk_substep / ddd_time_derivative calls on `stream`
 * advance a large ensemble as two contiguous half-ensembles on two internal
 * streams: half i of a call is ordered after everything enqueued on `stream`
 * before ddd_stream_fork and after half i of the previous call -- NOT after the
 * other half, so one half's launch boundary overlaps the other half's
 * evaluation.  Samples are independent, so results are bit-identical to the
 * unbracketed calls.  Contract inside the region: the arrays handed to these
 * calls are touched by nothing else (no other work on `stream` reads or writes
 * them, the host does not read them) until ddd_stream_join, after which `stream`
 * is ordered behind every substep enqueued.  Any other entry point taking this
 * model (and ddd_model_destroy) joins first, so a forgotten join cannot outlive
 * the model; calls on another stream, a batch too small to split, and models
 * without a per-equation MFMA kernel simply run on `stream` as without the
 * region.  ddd_stream_join without an open region is a no-op.  Neither call
 * synchronises the host.
 *
 * Round 6 -- the command ring (opt-in: ddd_set_region_mode(model, DDD_REGION_RING)).
 * Models with a per-equation MFMA kernel on one-wave groups (num_points divides 64;
 * default net) can run the region on ONE persistent kernel: the first ddd_rk_substep
 * of the region launches it on `stream`, and every call from then on is a 128-byte
 * command the host writes into a page-locked ring the kernel's wavefronts read -- no
 * launch, no drain, the conv weights stay in registers across calls.  Same contract as
 * above (the arrays belong to the region until the join), same bits as one launch per
 * call.  Measured at the rate of the launches (71.6 vs 71.1 % at 4 096 samples,
 * profiles/r6_ablation.txt), which is why it is not the default.  What differs:
 *   - work enqueued on `stream` INSIDE the region is ordered behind the persistent
 *     kernel, i.e. behind the join -- or behind the moment the region has been idle
 *     for 2 ms: a park thread then ends the kernel (the next call starts it again),
 *     so a caller that synchronises the device inside an open region waits that
 *     long, not for ever;
 *   - the host may run at most 256 calls ahead of the device; the 257th (and a join
 *     then) waits for room;
 *   - a host that stops for 20 s while the kernel waits (a debugger) trips the
 *     kernel's watchdog: the next call returns DDD_ERR_HIP and the region's results
 *     are undefined.
 * ddd_set_region_mode chooses: DDD_REGION_AUTO (default) and DDD_REGION_CHAINS = the
 * two chains of launches; DDD_REGION_RING = the ring where the model has one, else the
 * chains.  It closes an open region.  ddd_region_stats: persistent-kernel launches and
 * commands so far. */
enum ddd_region_mode { DDD_REGION_AUTO = 0, DDD_REGION_CHAINS = 1, DDD_REGION_RING = 2 };
DDD_API int ddd_stream_fork(ddd_model* model, void* stream);
DDD_API int ddd_stream_join(ddd_model* model, void* stream);
DDD_API int ddd_set_region_mode(ddd_model* model, int mode);
DDD_API int ddd_region_stats(const ddd_model* model, int64_t* ring_launches,
                             int64_t* ring_commands);

/* Replaces: model.integrate_ode (model.py:138-159) and, with the controller
 * pinned at max_step, the solve_ivp loop of integrate.odeint
 * (integrate.py:154-155) -- for the whole batch at once.
 * Advances n_steps steps of size dt from (t0, y0); every `save_every` steps
 * the state is written to y_out[(step+1)/save_every - 1][batch][N]
 * (n_steps / save_every snapshots).  y0 is not modified. */
DDD_API int ddd_integrate_fixed(ddd_model* model, int scheme, int launch_mode,
                        double t0, double dt, int n_steps, int save_every,
                        const float* y0, float* y_out, int batch, void* stream);

/* Same, integration state and I/O in float64 (right-hand side stays float32,
 * as in the reference where SciPy holds y in float64 and TF evaluates in
 * float32: integrate.py:57-60, 154).  Persistent launch mode only. */
DDD_API int ddd_integrate_fixed_f64(ddd_model* model, int scheme, double t0, double dt,
                            int n_steps, int save_every, const double* y0,
                            double* y_out, int batch, void* stream);

/* Replaces: integrate.odeint (integrate.py:143-169) =
 * scipy.integrate.solve_ivp(differentiator, (times[0], times[-1]), y0,
 * t_eval=times, max_step=0.01, method='RK23'), as scripts/run_evaluation.py
 * (:152-174) calls it once per sample -- for the whole batch in ONE launch,
 * with one SciPy-identical step-size controller per sample on the device:
 * Bogacki-Shampine 3(2) with FSAL, select_initial_step, error norm
 * RMS(err / (atol + rtol * max(|y|, |y_new|))), step factor
 * clip(0.9 * norm^(-1/3), 0.2, 10) without growth after a rejection, steps
 * clamped to [10 ulp(t), max_step], cubic dense output at `times`.  State,
 * controller and dense output in float64 (SciPy's), right-hand side in float32
 * fed float32(y), float32(t) (the TF placeholders, integrate.py:57-60).
 *   times  HOST [n_times], finite, strictly increasing; times[0] = t0 (the
 *          reference's rule: defaults rtol 1e-3, atol 1e-6, max_step 0.01)
 *   y0     [batch][N] float64;  y_out [n_times][batch][N] float64 (row 0 = y0)
 *   nfev   [batch] int32: right-hand-side evaluations of each sample
 *          (solve_ivp's sol.nfev)
 *   status [batch] int32: 0 = reached times[n_times-1]; -1 = step size fell
 *          below 10 ulp(t) (SciPy's "Required step size is less than spacing
 *          between numbers", sol.status -1); -2 = `max_attempts` steps tried
 *          (a safety net SciPy does not have; <= 0 selects a default of 1000x
 *          the attempts of a run at max_step).  Rows a failed sample did not
 *          reach are NaN, as integrate.odeint pads them (integrate.py:161-167).
 * Every model kind: MFMA-path models inside the persistent MFMA kernel; models
 * on the generic kernel (WENODifferentiator, integrate.py:124-140: the "exact"
 * Burgers solver; nets the MFMA path does not carry) with one workgroup per
 * sample; spectral models (ddd_spectral_create: SpectralDifferentiator, the
 * "exact" KdV / KS solver, integrate.py:108-121) with a float64 right-hand
 * side.  The spectral kernel carries no forcing term: a spectral model of the
 * Burgers family (whose finalize_time_derivative adds forcing(t),
 * equations.py:276-277) returns DDD_ERR_UNSUPPORTED here -- drive it from the host
 * over ddd_time_derivative_f64, as SpectralDifferentiator.__call__ does.
 * Enqueue-only: `times` is copied into a model-owned page-locked buffer before the
 * call returns (a ring of four; the host waits only if four adaptive calls on
 * this model are still in flight), uploaded and consumed on `stream`.  Not
 * capturable into a HIP graph (the ring recycles through events). */
DDD_API int ddd_integrate_adaptive_f64(ddd_model* model, const double* times,
                               int n_times, double rtol, double atol,
                               double max_step, long long max_attempts,
                               const double* y0, double* y_out, int32_t* nfev,
                               int32_t* status, int batch, void* stream);

/* Float64 forms for spectral models (ddd_spectral_create).
 * ddd_time_derivative_f64 replaces SpectralDifferentiator.__call__
 * (integrate.py:113-121) without finalize_time_derivative, batched;
 * ddd_rk_substep_f64 is ddd_rk_substep in float64:
 *   f = equation_of_motion(y_in);  y_out = y_base + c1 f;  acc_out = acc_in + c2 f
 * ddd_integrate_fixed_f64 on a spectral model steps with one fused launch per
 * substep, state and right-hand side in float64. */
DDD_API int ddd_time_derivative_f64(ddd_model* model, double t, const double* y,
                            double* dydt, int batch, void* stream);
DDD_API int ddd_rk_substep_f64(ddd_model* model, double t, const double* y_in,
                       const double* y_base, double c1, double* y_out,
                       const double* acc_in, double c2, double* acc_out,
                       int batch, void* stream);

/* Replaces: duckarray.smoothing_filter (duckarray.py:116-128), the low-pass
 * filter odeint_with_periodic_filtering (integrate.py:172-212) applies to the
 * state between segments and to the saved trajectory -- and any other
 * translation-invariant linear operator on the periodic grid.  Float64.
 *   out[r][x] = sum_j kernel[(x - j) mod n] * in[r][j],   r < rows
 * `kernel` [n] (device) is the operator applied to a unit impulse at x = 0
 * (smoothing_filter(delta, alpha, order)); in / out [rows][n]; out may alias in.
 * n <= 2048. */
DDD_API int ddd_circulant_apply_f64(const double* kernel, const double* in, double* out,
                            int rows, int n, void* stream);

/* ---- parity / debugging views of the same kernel ------------------------ */

/* Replaces: model.predict_space_derivatives (model.py:579-600) or
 * baseline_space_derivatives; out [batch][N][D]. */
DDD_API int ddd_space_derivatives(ddd_model* model, const float* y, float* out,
                          int batch, void* stream);

/* Replaces: model.predict_coefficients (model.py:420-513);
 * out [batch][N][D][G]. */
DDD_API int ddd_coefficients(ddd_model* model, const float* y, float* out, int batch,
                     void* stream);

/* ---- standalone operators (reference unit-test surface) ------------------ */

/* Replaces: layers.nn_conv1d_periodic / conv1d_periodic_layer
 * (layers.py:95-137).  in [batch][N][Cin], filters [K][Cin][Cout] (device),
 * bias [Cout] or NULL, out [batch][N][Cout]; activation -1 = none. */
DDD_API int ddd_conv1d_periodic(const float* in, const float* filters,
                        const float* bias, float* out, int batch, int n,
                        int cin, int cout, int k, int center, int activation,
                        void* stream);

/* Replaces: layers.pad_periodic (layers.py:39-83).
 * in [batch][N][C] -> out [batch][N + padding][C]. */
DDD_API int ddd_pad_periodic(const float* in, float* out, int batch, int n, int c,
                     int padding, int center, void* stream);

/* Replaces: model.extract_patches (model.py:516-533).
 * in [batch][N] -> out [batch][N][size], out[b][x][i] = in[b][(x + i - size/2) mod N]. */
DDD_API int ddd_extract_patches(const float* in, float* out, int batch, int n, int size,
                        void* stream);

/* Replaces: model.apply_coefficients (model.py:536-548).
 * coefficients [batch][N][D][G], in [batch][N] -> out [batch][N][D]. */
DDD_API int ddd_apply_coefficients(const float* coefficients, const float* in, float* out,
                           int batch, int n, int d, int g, void* stream);

/* Replaces: model.apply_space_derivatives (model.py:115-135):
 * Equation.equation_of_motion on given derivatives [batch][N][D] (order of
 * DERIVATIVE_NAMES) and the state y [batch][N] -> time derivative [batch][N],
 * without finalize_time_derivative.  `equation` is a ddd_equation. */
DDD_API int ddd_apply_space_derivatives(int equation, const float* derivatives, const float* y,
                                float* out, int batch, int n, int d, double eta,
                                double dx, void* stream);

/* Replaces: PolynomialAccuracyLayer.apply (polynomials.py:266-277).
 * inputs [m][input_size], nullspace [input_size][G], bias [G], out [m][G]. */
DDD_API int ddd_polynomial_accuracy_apply(const float* inputs, const float* nullspace,
                                  const float* bias, float* out, int64_t m,
                                  int input_size, int g, void* stream);

/* ---- training ------------------------------------------------------------
 * Replaces: the loss and its gradient of training.setup_training
 * (training.py:337-370) on one minibatch, i.e. model.predict_result
 * (model.py:664-697), abs_and_rel_error / loss_per_head / weighted_loss
 * (model.py:704-810) and tf.gradients of that loss with respect to the conv
 * kernels and biases.  Stateless: no ddd_model is involved, the weights are a
 * device vector in the layout ddd_model_create documents (per layer the kernel
 * [K][Cin][Cout] then the bias [Cout]) and may change between calls.
 * H = num_derivatives + 1 heads in result_stack order: the space derivatives,
 * then the time derivative (equation_of_motion, no forcing).
 * Supported: the six non-Godunov equations; model_target coefficients (any
 * polynomial_accuracy_order >= 0), space_derivatives or time_derivative;
 * 1 <= num_layers <= DDD_MAX_LAYERS, kernel_size <= 7, filter_size <= 64,
 * 8 <= num_points <= 256.  Other configurations return DDD_ERR_UNSUPPORTED
 * before any device work. */
#define DDD_MAX_HEADS (DDD_MAX_DERIVATIVES + 1)

typedef struct ddd_train_args {
  int32_t struct_size;   /* = sizeof(ddd_train_args), checked */
  int32_t batch;         /* samples in the minibatch */
  int32_t num_rows;      /* S: rows of y / labels / baseline */
  int32_t reserved0;
  const float* weights;  /* conv weights (ddd_model_create layout) */
  const float* nullspace; /* [sum(input_sizes)][G], coefficients target with
                             accuracy order > 0, else NULL */
  const float* bias;     /* [D][G], same condition */
  const float* y;        /* [S][N] coarse inputs */
  const int32_t* sample_index; /* [batch] rows of the minibatch, NULL = 0..batch-1.
                                  An index outside [0, S) makes head_means and
                                  that sample's predictions row NaN. */
  const float* labels;   /* [S][N][H] */
  const float* baseline; /* [S][N][H] */
  float error_floor[DDD_MAX_HEADS]; /* HOST values, first H used */
  float coef_abs[DDD_MAX_HEADS];    /* loss = sum_h coef_abs[h] mean_abs[h] */
  float coef_rel[DDD_MAX_HEADS];    /*      + coef_rel[h] mean_rel[h]       */
  float* head_means;     /* out [2][H]: batch means of model_error / relative_error */
  float* grad;           /* out, layout of `weights`; NULL = forward and loss only */
  float* predictions;    /* out [batch][N][H] or NULL */
  void* workspace;       /* ddd_train_workspace_bytes(cfg, batch) bytes */
  size_t workspace_bytes;
} ddd_train_args;

/* Bytes of the caller-allocated workspace of ddd_train_loss_grad for `batch`
 * samples (partial gradient slabs and per-workgroup scratch); 0 on error. */
DDD_API size_t ddd_train_workspace_bytes(const ddd_config* cfg, int batch);
/* head_means and, with grad non-NULL, the gradient of
 * sum_h coef_abs[h] head_means[0][h] + coef_rel[h] head_means[1][h] with respect to
 * every conv kernel and bias.  Deterministic: each workgroup owns fixed samples and
 * a partial slab, the slabs are summed in a fixed order (no atomics), so equal
 * inputs give bit-identical outputs.  error_max clipping (tf.where passes no
 * gradient through a clipped head) is two calls: grad = NULL first, then the
 * clipped heads' coefficients zeroed. */
DDD_API int ddd_train_loss_grad(const ddd_config* cfg, const ddd_train_args* args,
                                void* stream);

/* ---- training through time ------------------------------------------------
 * Replaces: the same loss with hparams.num_time_steps = T > 0, i.e. with
 * model.predict_time_evolution (model.py:643-661) appended to predict_result
 * (model.py:686-696): T more heads, the model's own midpoint-rule trajectory
 * y(t_1) .. y(t_T) from the input row with step `time_step` (the equation of
 * motion without forcing), compared with the integrated_solution channels of
 * the labels.  H' = num_derivatives + 1 + T heads in result_stack order: the
 * space derivatives, the time derivative, then y(t_1) .. y(t_T).  One launch
 * runs the 2 T evaluations of the unroll forward and the adjoint of the
 * midpoint rule backward, per sample, plus the fixed-order slab sum.
 * Supports exactly the configurations ddd_train_loss_grad supports (same
 * messages), with 1 <= T <= DDD_MAX_TIME_STEPS. */
#define DDD_MAX_TIME_STEPS 8
#define DDD_MAX_UNROLLED_HEADS (DDD_MAX_HEADS + DDD_MAX_TIME_STEPS)

typedef struct ddd_train_unrolled_args {
  int32_t struct_size;   /* = sizeof(ddd_train_unrolled_args), checked */
  int32_t batch;         /* samples in the minibatch */
  int32_t num_rows;      /* S: rows of y / labels / baseline */
  int32_t num_time_steps; /* T */
  const float* weights;  /* as ddd_train_args */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y;        /* [S][N] coarse inputs */
  const int32_t* sample_index; /* as ddd_train_args */
  const float* labels;   /* [S][N][H'] */
  const float* baseline; /* [S][N][H'] */
  float time_step;       /* the equation's time_step */
  float error_floor[DDD_MAX_UNROLLED_HEADS]; /* HOST values, first H' used */
  float coef_abs[DDD_MAX_UNROLLED_HEADS];
  float coef_rel[DDD_MAX_UNROLLED_HEADS];
  float* head_means;     /* out [2][H'] */
  float* grad;           /* out, layout of `weights`; NULL = forward and loss only */
  float* predictions;    /* out [batch][N][H'] or NULL */
  void* workspace;       /* ddd_train_unrolled_workspace_bytes(cfg, batch, T) bytes */
  size_t workspace_bytes;
} ddd_train_unrolled_args;

/* Bytes of the caller-allocated workspace of ddd_train_unrolled_loss_grad
 * (partial gradient slabs, per-workgroup scratch and stage states); 0 on error. */
DDD_API size_t ddd_train_unrolled_workspace_bytes(const ddd_config* cfg, int batch,
                                                  int num_time_steps);
/* head_means and, with grad non-NULL, the gradient of
 * sum_h coef_abs[h] head_means[0][h] + coef_rel[h] head_means[1][h] over all H'
 * heads with respect to every conv kernel and bias.  Deterministic, sample_index,
 * grad = NULL, predictions = NULL and error_max clipping as ddd_train_loss_grad. */
DDD_API int ddd_train_unrolled_loss_grad(const ddd_config* cfg,
                                         const ddd_train_unrolled_args* args, void* stream);

/* ---- training on rollout error ----------------------------------------------
 * The loss is the error of a rollout itself: from each window start y0 the model's
 * own midpoint-rule trajectory over T = num_steps steps of size dt, FORCED as the
 * equation is forced, compared at every save_every-th step with given targets
 * (e.g. the coarse-grained exact solution), and the gradient of that loss with
 * respect to every conv kernel and bias, in one launch plus the fixed-order slab
 * sum.  Per window (row):
 *   y_{s+1} = y_s + dt f(t_s + dt/2, y_s + (dt/2) f(t_s, y_s)),
 *   f(t, y) = the time derivative of ddd_train_loss_grad's last head (equation of
 *             motion) + forcing_row(x, t), the forcing of ddd_set_forcing in the
 *             same float32 order, added after the flux difference; t is formed in
 *             float64 as t0[row] + s dt (+ dt/2) and rounded to float32.  Ignored
 *             by KdV and KS, as ddd_set_forcing documents.
 *   step_means[j] = mean over (sample, x) of (y_{(j+1) save_every} - targets[j])^2
 *   loss = sum_j step_weights[j] step_means[j]
 * The forcing depends on neither the state nor the weights: the adjoint is that of
 * ddd_train_unrolled_loss_grad with cotangents entering at saved steps only, and
 * an unforced call with save_every = 1 repeats that entry point's integrated
 * heads bit for bit.  All 2 T stage states of a window are kept in the workspace
 * (2 T N floats per workgroup, at most 512 workgroups) next to the saved-step
 * cotangents; the loss constants are a DEVICE array, so T is not tied to
 * DDD_MAX_TIME_STEPS.  Supports exactly the configurations ddd_train_loss_grad
 * supports, named "ddd_train_rollout_loss_grad" in the messages.
 * DDD_ERR_INVALID_ARGUMENT: num_steps outside [1, DDD_MAX_ROLLOUT_STEPS],
 * save_every < 1 or not a divisor of num_steps, dt <= 0, a struct_size mismatch,
 * NULL y0 / targets / step_weights / step_means, forcing pointers partly given. */
#define DDD_MAX_ROLLOUT_STEPS 256

typedef struct ddd_train_rollout_args {
  int32_t struct_size;   /* = sizeof(ddd_train_rollout_args), checked */
  int32_t batch;         /* windows in the minibatch */
  int32_t num_rows;      /* S: rows of y0 / targets / t0 / the forcing tables */
  int32_t num_steps;     /* T */
  int32_t save_every;    /* a divisor of T; T / save_every saved steps */
  const float* weights;  /* as ddd_train_args */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y0;       /* device [S][N] window starts */
  const int32_t* sample_index; /* as ddd_train_args: an index outside [0, S) makes
                                  step_means and that sample's trajectory rows NaN */
  const float* targets;  /* device [S][T / save_every][N] */
  const float* step_weights; /* device [T / save_every]: c_j */
  double dt;             /* step of the midpoint rule */
  const double* t0;      /* device [S]: start time per row, NULL = 0 */
  /* forcing, one row per row of y0: the tables of ddd_set_forcing as DEVICE arrays;
   * amplitude NULL (then all five NULL) = unforced.  A k_index outside [0, n_k)
   * reads nothing and makes that row's trajectory NaN. */
  int32_t nparams, n_k;
  const float* amplitude;     /* [S][nparams] */
  const float* omega;         /* [S][nparams] */
  const float* phase;         /* [S][nparams] */
  const int32_t* k_index;     /* [S][nparams] */
  const float* spatial_phase; /* [n_k][N] */
  float* step_means;     /* out [T / save_every] */
  float* grad;           /* out, layout of `weights`; NULL = forward and loss only */
  float* trajectory;     /* out [batch][T / save_every][N] or NULL */
  void* workspace;       /* ddd_train_rollout_workspace_bytes(cfg, batch, T) bytes */
  size_t workspace_bytes;
} ddd_train_rollout_args;

/* Bytes of the caller-allocated workspace of ddd_train_rollout_loss_grad for any
 * save_every (partial gradient slabs, per-workgroup scratch, stage states and
 * saved-step cotangents); 0 on an unsupported configuration or num_steps out of range. */
DDD_API size_t ddd_train_rollout_workspace_bytes(const ddd_config* cfg, int batch,
                                                 int num_steps);
/* step_means and, with grad non-NULL, the gradient of sum_j step_weights[j]
 * step_means[j] with respect to every conv kernel and bias.  Deterministic,
 * sample_index, grad = NULL and trajectory = NULL as ddd_train_unrolled_loss_grad
 * (there: predictions). */
DDD_API int ddd_train_rollout_loss_grad(const ddd_config* cfg,
                                        const ddd_train_rollout_args* args, void* stream);

/* ---- the optimiser loop on the device --------------------------------------
 * Replaces: num_steps iterations of training.training_loop (training.py:570-636)
 * between two evaluations: per step the loss and gradient of
 * ddd_train_loss_grad (num_time_steps = 0) or ddd_train_unrolled_loss_grad
 * (1 <= num_time_steps <= DDD_MAX_TIME_STEPS) on that step's minibatch, then
 * tf.train.AdamOptimizer's update, which is the single-tensor path of
 * torch.optim.Adam without weight decay or amsgrad, in float32 and in this order:
 *   m += (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *   denom = sqrt(v) / sqrt(1 - beta2^t) + epsilon;  w -= (lr / (1 - beta1^t)) m / denom
 * for t = first_step + k + 1 at step k (lr / (1 - beta1^t) and sqrt(1 - beta2^t) are
 * formed on the host in double).  One call enqueues every step on `stream` and
 * returns: no stream synchronisation, no copy to the host, no graph capture.  The
 * update is fused into the kernel that sums the gradient slabs, in their fixed
 * order, so the gradient of a step is bit for bit what the two entry points above
 * return for the same weights and minibatch, and equal inputs give equal bits.
 * error_max > 0 is decided on the device: per step a forward-only pass, then the
 * coefficient of every term with head_mean * error_scale >= error_max (compared in
 * double) zeroed for the pass that forms the gradient, as the two-call path of
 * ddd_train_loss_grad does on the host.  The logged means are the unclipped ones.
 * H' = num_derivatives + 1 + num_time_steps heads.  Supports exactly the
 * configurations ddd_train_loss_grad supports and refuses the others with the same
 * status and text ("training run" as the entry point's name). */
typedef struct ddd_train_run_args {
  int32_t struct_size;   /* = sizeof(ddd_train_run_args), checked */
  int32_t batch;         /* samples per minibatch */
  int32_t num_rows;      /* S: rows of y / labels / baseline */
  int32_t num_time_steps; /* T; 0 = the loss of ddd_train_loss_grad */
  int32_t first_step;    /* optimiser steps already taken (>= 0) */
  int32_t num_steps;     /* optimiser steps of this call (>= 1) */
  float* weights;        /* in/out: conv weights (ddd_model_create layout) */
  float* adam_m;         /* in/out, layout of `weights`: first moment */
  float* adam_v;         /* in/out, layout of `weights`: second moment */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y;        /* [S][N] coarse inputs */
  const int32_t* sample_index; /* device [num_steps][batch], required: step k trains
                                  on rows sample_index[k][0 .. batch-1].  An index
                                  outside [0, S) makes that step's logged means NaN
                                  and, through the update (the gradient is NaN too),
                                  the weights, adam_m and adam_v
                                  (ddd_train_loss_grad: head_means NaN). */
  const float* labels;   /* [S][N][H'] */
  const float* baseline; /* [S][N][H'] */
  const double* learning_rate; /* HOST [num_steps], finite and >= 0 */
  double beta1, beta2;   /* in [0, 1) */
  double epsilon;        /* > 0 */
  double error_max;      /* 0 = no clipping */
  double error_scale_abs[DDD_MAX_UNROLLED_HEADS]; /* HOST, first H' used, read with */
  double error_scale_rel[DDD_MAX_UNROLLED_HEADS]; /* error_max > 0 only            */
  float error_floor[DDD_MAX_UNROLLED_HEADS]; /* HOST values, first H' used */
  float coef_abs[DDD_MAX_UNROLLED_HEADS];
  float coef_rel[DDD_MAX_UNROLLED_HEADS];
  float time_step;       /* the equation's time_step (T > 0) */
  float* head_means_log; /* out [num_steps][2][H']: every step's head_means */
  float* last_grad;      /* out, layout of `weights`, or NULL: the last step's gradient */
  void* workspace;       /* ddd_train_run_workspace_bytes(cfg, batch, T) bytes */
  size_t workspace_bytes;
} ddd_train_run_args;

/* Bytes of the caller-allocated workspace of ddd_train_run: that of
 * ddd_train_workspace_bytes (T = 0) or ddd_train_unrolled_workspace_bytes plus the
 * device table of loss constants; depends only on cfg, batch and T.  0 on error. */
DDD_API size_t ddd_train_run_workspace_bytes(const ddd_config* cfg, int batch,
                                             int num_time_steps);
/* Enqueues num_steps optimiser steps.  Arguments are checked before any device work. */
DDD_API int ddd_train_run(const ddd_config* cfg, const ddd_train_run_args* args,
                          void* stream);

/* ---- replica populations ---------------------------------------------------
 * Replaces: R runs of training.training_loop that differ in the initial seed and
 * the learning-rate schedule (the shape in which the reference's models are
 * compared).  ddd_train_run on R replicas of one architecture in one call: R weight
 * vectors, R Adam states, R learning-rate rows and, with index_per_replica, R
 * minibatch orders, over one dataset.  The replicas are a second grid dimension of
 * the same kernels, so a step is the same number of launches whatever R is, and each
 * replica keeps the workgroups, slabs and summation order of a solo run: replica r of
 * a call is bit for bit ddd_train_run given replica r's weights, state, learning
 * rates and index (weights, adam_m, adam_v, every log row and last_grad).  With
 * error_max > 0 every replica clips from its own forward-only means.  Shared by all
 * replicas: the dataset, nullspace / bias, first_step, the betas, epsilon, error_max,
 * the loss constants and time_step.  Supports exactly the configurations
 * ddd_train_run supports and refuses the others with the same status and text
 * ("training population" as the entry point's name). */
#define DDD_MAX_REPLICAS 64

typedef struct ddd_train_population_args {
  int32_t struct_size;   /* = sizeof(ddd_train_population_args), checked */
  int32_t batch;         /* samples per minibatch */
  int32_t num_rows;      /* S: rows of y / labels / baseline */
  int32_t num_time_steps; /* T; 0 = the loss of ddd_train_loss_grad */
  int32_t first_step;    /* optimiser steps already taken (>= 0), of every replica */
  int32_t num_steps;     /* optimiser steps of this call (>= 1) */
  int32_t replicas;      /* R in [1, DDD_MAX_REPLICAS] */
  int32_t index_per_replica; /* 0: one minibatch order for all; 1: one per replica */
  float* weights;        /* in/out [R][n_weights] (ddd_model_create layout per row) */
  float* adam_m;         /* in/out [R][n_weights] */
  float* adam_v;         /* in/out [R][n_weights] */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y;        /* [S][N] coarse inputs */
  const int32_t* sample_index; /* device [num_steps][batch], or [num_steps][R][batch]
                                  with index_per_replica.  An index outside [0, S)
                                  makes that step's logged means NaN and, through
                                  the update (the gradient is NaN too), the weights,
                                  adam_m and adam_v, of the replicas that read it
                                  only. */
  const float* labels;   /* [S][N][H'] */
  const float* baseline; /* [S][N][H'] */
  const double* learning_rate; /* HOST [R][num_steps], finite and >= 0 */
  double beta1, beta2;   /* in [0, 1) */
  double epsilon;        /* > 0 */
  double error_max;      /* 0 = no clipping */
  double error_scale_abs[DDD_MAX_UNROLLED_HEADS]; /* HOST, first H' used, read with */
  double error_scale_rel[DDD_MAX_UNROLLED_HEADS]; /* error_max > 0 only            */
  float error_floor[DDD_MAX_UNROLLED_HEADS]; /* HOST values, first H' used */
  float coef_abs[DDD_MAX_UNROLLED_HEADS];
  float coef_rel[DDD_MAX_UNROLLED_HEADS];
  float time_step;       /* the equation's time_step (T > 0) */
  float* head_means_log; /* out [num_steps][R][2][H'] */
  float* last_grad;      /* out [R][n_weights] or NULL: the last step's gradients */
  void* workspace;       /* ddd_train_population_workspace_bytes(cfg, batch, T, R) bytes */
  size_t workspace_bytes;
} ddd_train_population_args;

/* Bytes of the caller-allocated workspace of ddd_train_population_run: `replicas`
 * times ddd_train_run_workspace_bytes(cfg, batch, T) (R times the slabs, then R
 * coefficient tables).  0 on error, replicas outside [1, DDD_MAX_REPLICAS] included. */
DDD_API size_t ddd_train_population_workspace_bytes(const ddd_config* cfg, int batch,
                                                    int num_time_steps, int replicas);
/* Enqueues num_steps optimiser steps of every replica: no stream synchronisation, no
 * copy to the host, no graph capture.  Arguments are checked before any device work. */
DDD_API int ddd_train_population_run(const ddd_config* cfg,
                                     const ddd_train_population_args* args, void* stream);

/* ---- rollout fine-tuning on the device, for replica populations --------------
 * Replaces: num_opt_steps iterations of training.RolloutTrainer.step per replica:
 * per step the loss and gradient of ddd_train_rollout_loss_grad on that step's
 * minibatch of windows, the gradient's global norm, the skip of a step whose
 * norm is not finite, the rescaling to clip_norm and Adam, for R replicas of one
 * architecture over one set of windows.  One call enqueues every step on `stream`
 * and returns: no stream synchronisation, no copy to the host, no graph capture.
 * A step is four launches whatever R is (the replicas are a second grid dimension),
 * and each replica keeps the workgroups, slabs and summation order of a solo run:
 *   - the gradient of a step (last_grad) and its step means are bit for bit what
 *     ddd_train_rollout_loss_grad returns for the same weights and minibatch;
 *   - norm = sqrt(sum g^2), summed in float64 in a fixed order; grad_norm_log holds
 *     (float) norm, before clipping.  Not finite: the step is SKIPPED for this
 *     replica: weights, adam_m, adam_v and adam_step keep their bits;
 *   - otherwise g' = g * (float) min(1, clip_norm / (norm + 1e-12)) (clip_norm = 0:
 *     g' = g), t = ++adam_step[r], and the update of ddd_train_run in float32:
 *       m += (g' - m) (1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
 *       denom = sqrt(v) / sqrt(1 - beta2^t) + epsilon;  w -= (lr / (1 - beta1^t)) m / denom
 *     lr / (1 - beta1^t) and sqrt(1 - beta2^t) are formed ON THE DEVICE in double and
 *     rounded to float: skips are per replica and decided there, so t lives on the
 *     device.  The device's pow may differ from the host's by an ulp of double; what
 *     is bit for bit is so between runs on the device: replica r of a call equals
 *     the call with that replica alone (weights, adam_m, adam_v, adam_step, every
 *     log row and last_grad), K steps in one call equal the same steps in several.
 * An index outside [0, S) makes that step's means and gradient NaN for the
 * replicas that read it, which skips their step.  Supports exactly the
 * configurations ddd_train_rollout_loss_grad supports and refuses the others with
 * the same status and text ("ddd_train_rollout_run" as the entry point's name).
 * DDD_ERR_INVALID_ARGUMENT: a struct_size mismatch; replicas, num_opt_steps,
 * num_steps or save_every out of range; dt <= 0; clip_norm negative or not finite;
 * a beta outside [0, 1); epsilon <= 0; a learning rate negative or not finite; a
 * required pointer NULL; forcing pointers partly given; a workspace too small.
 *
 * forward_only = 1 (num_opt_steps must be 1): one loss pass without gradient per
 * replica fills step_means_log[0]; nothing else is written.  sample_index may be
 * NULL (all rows, batch = num_rows); learning_rate, adam_* and grad_norm_log may
 * be NULL. */
typedef struct ddd_train_rollout_run_args {
  int32_t struct_size;   /* = sizeof(ddd_train_rollout_run_args), checked */
  int32_t batch;         /* windows per minibatch */
  int32_t num_rows;      /* S: rows of y0 / targets / t0 / the forcing tables */
  int32_t num_steps;     /* T in [1, DDD_MAX_ROLLOUT_STEPS] */
  int32_t save_every;    /* a divisor of T; T / save_every saved steps */
  int32_t num_opt_steps; /* K >= 1: optimiser steps of this call */
  int32_t replicas;      /* R in [1, DDD_MAX_REPLICAS] */
  int32_t index_per_replica; /* 0: one minibatch order for all; 1: one per replica */
  int32_t forward_only;  /* 0 or 1 */
  float* weights;        /* in/out [R][n_weights] (ddd_model_create layout per row) */
  float* adam_m;         /* in/out [R][n_weights] */
  float* adam_v;         /* in/out [R][n_weights] */
  int32_t* adam_step;    /* in/out DEVICE [R]: updates applied so far (>= 0) */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  /* the windows, shared by all replicas, as in ddd_train_rollout_args */
  const float* y0;       /* device [S][N] */
  const float* targets;  /* device [S][T / save_every][N] */
  const float* step_weights; /* device [T / save_every] */
  double dt;
  const double* t0;      /* device [S] or NULL (0) */
  int32_t nparams, n_k;
  const float* amplitude;     /* [S][nparams]; all five NULL = unforced */
  const float* omega;         /* [S][nparams] */
  const float* phase;         /* [S][nparams] */
  const int32_t* k_index;     /* [S][nparams] */
  const float* spatial_phase; /* [n_k][N] */
  const int32_t* sample_index; /* device [K][batch], or [K][R][batch] with
                                  index_per_replica */
  const double* learning_rate; /* HOST [R][K], finite and >= 0 */
  double beta1, beta2;   /* in [0, 1) */
  double epsilon;        /* > 0 */
  double clip_norm;      /* >= 0, finite; 0 = no clipping */
  float* step_means_log; /* out [K][R][T / save_every] */
  float* grad_norm_log;  /* out [K][R]: the norm before clipping; not finite = the
                            step was skipped */
  float* last_grad;      /* out [R][n_weights] or NULL: the last step's gradients,
                            before clipping */
  void* workspace;       /* ddd_train_rollout_run_workspace_bytes(cfg, batch, T, R) bytes */
  size_t workspace_bytes;
} ddd_train_rollout_run_args;

/* Bytes of the caller-allocated workspace of ddd_train_rollout_run: `replicas` times
 * ddd_train_rollout_workspace_bytes(cfg, batch, T), then the gradient buffers, the
 * partial sums of the norms and the decision records.  Depends only on cfg, batch, T
 * and R.  0 on error, replicas outside [1, DDD_MAX_REPLICAS] included. */
DDD_API size_t ddd_train_rollout_run_workspace_bytes(const ddd_config* cfg, int batch,
                                                     int num_steps, int replicas);
/* Enqueues num_opt_steps optimiser steps of every replica (or the forward-only pass).
 * Arguments are checked before any device work. */
DDD_API int ddd_train_rollout_run(const ddd_config* cfg,
                                  const ddd_train_rollout_run_args* args, void* stream);

/* ---- evaluation on the device -----------------------------------------------
 * Replaces: training.Inferer.run + calculate_metrics (training.py:253-314,
 * 433-491) for R replicas of one architecture over one dataset: forward only,
 * two launches whatever R is.  Per replica and head h of the H' =
 * num_derivatives + 1 + num_time_steps heads, over the rows evaluated and their
 * N points, with prediction p, label l and baseline b:
 *   sums[r][0][h], sums[r][1][h]  head_means of ddd_train_loss_grad /
 *                                 ddd_train_unrolled_loss_grad (grad = NULL) on the
 *                                 same rows, bit for bit (means over rows N)
 *   sums[r][2][h], sums[r][3][h]  sum |l - p|, sum |l - b|
 *   sums[r][4][h], sums[r][5][h]  sum (l - p)^2, sum (l - b)^2
 *   sums[r][6][h]                 sum log(max(|l - p|, 1e-8)) - log(max(|l - b|, 1e-8))
 *   below[r][h]                   points with (l - p)^2 < (l - b)^2, counted in int32
 *                                 (rows_evaluated N < 2^31)
 * all in float32, each workgroup's samples in a fixed order and the workgroups'
 * partial sums in a fixed order (no atomics): equal inputs give equal bits, and
 * replica r of a call equals the call on replica r alone.  The ratios, roots and
 * exponentials of the metrics are the caller's.  Supports exactly the
 * configurations ddd_train_loss_grad supports and refuses the others with the same
 * status and text ("evaluation metrics" as the entry point's name). */
typedef struct ddd_eval_metrics_args {
  int32_t struct_size;   /* = sizeof(ddd_eval_metrics_args), checked */
  int32_t rows_evaluated; /* B: samples evaluated per replica */
  int32_t num_rows;      /* S: rows of y / labels / baseline */
  int32_t num_time_steps; /* T; 0 = the heads of ddd_train_loss_grad */
  int32_t replicas;      /* R in [1, DDD_MAX_REPLICAS] */
  int32_t index_per_replica; /* 0: one sample_index for all; 1: one per replica */
  const float* weights;  /* [R][n_weights] (ddd_model_create layout per row) */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y;        /* [S][N] coarse inputs */
  const int32_t* sample_index; /* device [B], or [R][B] with index_per_replica, or NULL
                                  (rows 0 .. B-1, B <= S).  An index outside [0, S)
                                  makes the sums NaN and the counts -1 of the replicas
                                  that read it, and that sample's predictions row NaN;
                                  no input is read for it. */
  const float* labels;   /* [S][N][H'] */
  const float* baseline; /* [S][N][H'] */
  float error_floor[DDD_MAX_UNROLLED_HEADS]; /* HOST values, first H' used */
  float coef_abs[DDD_MAX_UNROLLED_HEADS];    /* (accepted for symmetry with training; */
  float coef_rel[DDD_MAX_UNROLLED_HEADS];    /*  the sums do not depend on them)      */
  float time_step;       /* the equation's time_step (T > 0) */
  float* sums;           /* out [R][7][H'] */
  int32_t* below;        /* out [R][H'] */
  float* predictions;    /* out [R][B][N][H'] or NULL */
  void* workspace;       /* ddd_eval_metrics_workspace_bytes(cfg, B, T, R) bytes */
  size_t workspace_bytes;
} ddd_eval_metrics_args;

/* Bytes of the caller-allocated workspace of ddd_eval_metrics (per replica and
 * workgroup the partial sums, the scratch of the forward pass and the stage states).
 * 0 on error, replicas outside [1, DDD_MAX_REPLICAS] included. */
DDD_API size_t ddd_eval_metrics_workspace_bytes(const ddd_config* cfg, int rows_evaluated,
                                                int num_time_steps, int replicas);
/* Enqueues the two launches: no stream synchronisation, no copy to the host, no graph
 * capture.  Arguments are checked before any device work. */
DDD_API int ddd_eval_metrics(const ddd_config* cfg, const ddd_eval_metrics_args* args,
                             void* stream);

/* ---- rollout scores on the device -------------------------------------------
 * Replaces: the scoring of scripts/run_evaluation.py:181-216 over analysis.py:39-90
 * (unify_x_coords, is_good, mostly_good, calculate_survival, mostly_good_survival
 * and the mean absolute error up to each stop time), which the reference runs on
 * the host per model over whole [sample, time, x] trajectories.  Here the exact
 * data is block-averaged once on the device (ddd_rollout_reference) and the
 * trajectories of R replicas, as the integrators wrote them, are scored where they
 * are (ddd_rollout_scores: two launches whatever R is).  Stateless: no model
 * handle, no ddd_config. */
#define DDD_ROLLOUT_MAX_QUANTILES 8
#define DDD_ROLLOUT_MAX_STOP_TIMES 16
#define DDD_ROLLOUT_MAX_POINTS 1024
#define DDD_ROLLOUT_MAX_FACTOR 128
#define DDD_ROLLOUT_F64 0 /* y_model is float64 (the adaptive integrator's output) */
#define DDD_ROLLOUT_F32 1 /* y_model is float32 (the fixed-step integrator's) */

typedef struct ddd_rollout_reference_args {
  int32_t struct_size;   /* = sizeof(ddd_rollout_reference_args), checked */
  int32_t num_samples;   /* S >= 1 */
  int32_t num_times;     /* T >= 1 */
  int32_t num_points_exact; /* X = f N, 1 <= f <= DDD_ROLLOUT_MAX_FACTOR */
  int32_t num_points;    /* N in [1, DDD_ROLLOUT_MAX_POINTS] */
  const double* y_exact; /* device [S][T][X] */
  double* exact_low;     /* out, device [T][S][N] (the layout of the trajectories) */
} ddd_rollout_reference_args;

/* exact_low[t][s][j] = mean of y_exact[s][t][j f .. j f + f - 1], added in the order
 * numpy.mean uses on a contiguous last axis (below eight values left to right; else
 * eight accumulators over the full groups of eight, combined as a balanced tree, then
 * the remaining f mod 8 values left to right; one division by f): bit for bit
 * analysis.unify_x_coords, and row t = 0 is run_evaluation.py's
 * load_initial_conditions.  One launch, enqueued on `stream`: no synchronisation, no
 * copy to the host, no graph capture.  Arguments are checked before any device work. */
DDD_API int ddd_rollout_reference(const ddd_rollout_reference_args* args, void* stream);

/* With e = |y_model - exact_low| in float64 (a float32 y_model converted first):
 *   row_abs_sum[r][t][s] = sum over x of e
 *   good[r][q][t][s]     = ((double)#{x : e <= max_error[q]} / (double)N) >= frac_good[q]
 *                          (is_good(...).mean(-1) >= frac_good; a NaN point is not good)
 *   survival[r][q][s]    = times[first t with good == 0], times[T-1] if there is none
 *   mae[r][k][s]         = (sum of row_abs_sum over the t with times[t] <= stop_times[k],
 *                          in time order) / (their number N); NaN if a row kept is NaN
 *                          or none is kept
 * Each row is summed in an order that depends on N alone and there are no atomics:
 * equal inputs give equal bits, and replica r of a call equals the call on replica r
 * alone. */
typedef struct ddd_rollout_scores_args {
  int32_t struct_size;   /* = sizeof(ddd_rollout_scores_args), checked */
  int32_t replicas;      /* R in [1, DDD_MAX_REPLICAS] */
  int32_t num_times;     /* T >= 1 */
  int32_t num_samples;   /* S >= 1 */
  int32_t num_points;    /* N in [1, DDD_ROLLOUT_MAX_POINTS] */
  int32_t num_quantiles; /* Q in [1, DDD_ROLLOUT_MAX_QUANTILES] */
  int32_t num_stop_times; /* K in [1, DDD_ROLLOUT_MAX_STOP_TIMES] */
  int32_t dtype;         /* DDD_ROLLOUT_F64 or DDD_ROLLOUT_F32: the type of y_model */
  const void* y_model;   /* device [R][T][S][N] */
  const double* exact_low; /* device [T][S][N] */
  const double* times;   /* HOST [T], finite and strictly increasing */
  const double* max_error; /* HOST [Q] */
  const double* frac_good; /* HOST [Q] */
  const double* stop_times; /* HOST [K] */
  double* mae;           /* out, device [R][K][S] */
  double* survival;      /* out, device [R][Q][S] */
  double* row_abs_sum;   /* out, device [R][T][S], or NULL */
  uint8_t* good;         /* out, device [R][Q][T][S], or NULL */
  void* workspace;       /* ddd_rollout_scores_workspace_bytes(R, T, S, Q) bytes, device,
                            8-byte aligned */
  size_t workspace_bytes;
} ddd_rollout_scores_args;

/* Bytes of the caller-allocated workspace of ddd_rollout_scores (the row sums, the
 * good flags and the times); 0 on error, replicas outside [1, DDD_MAX_REPLICAS]
 * included. */
DDD_API size_t ddd_rollout_scores_workspace_bytes(int replicas, int num_times, int num_samples,
                                                  int num_quantiles);
/* Enqueues a copy of `times` (through a page-locked buffer of the library's: the
 * caller's arrays are free on return) and the two launches: no stream synchronisation,
 * no copy to the host, no graph capture.  Arguments are checked before any device
 * work. */
DDD_API int ddd_rollout_scores(const ddd_rollout_scores_args* args, void* stream);

/* ---- rollouts of a replica population in one launch ------------------------
 * R models of ONE architecture that differ only in their weights, integrated by one
 * launch whose grid is (groups, R): workgroup (g, r) is group g of a solo launch on
 * `batch` samples, run with replica r's weights.  Replica r's part of every output is
 * bit for bit what ddd_integrate_adaptive_f64 / ddd_integrate_fixed (persistent launch
 * mode) writes for models[r] alone from the same y0, NaN rows included.
 *
 * ddd_population_create takes 1 <= replicas <= DDD_MAX_REPLICAS distinct model handles
 * with identical ddd_config (equation, grid, tower, head, standard deviation; of
 * derivative_orders[] and input_sizes[] the num_derivatives entries in use, reserved[] not
 * at all) and equal projection tables, and copies each model's packed weights device to device: a later
 * change to a model does not reach the population.  Carried: models on the MFMA route
 * with the per-equation specialisation of the one-wavefront kernels, num_points dividing
 * 64, no explicit ddd_set_kernel choice.  Everything else (num_points not dividing 64 --
 * the 256-row geometry --, the run-time-parameterised, wide, other-tower and 16-channel-
 * tile kernels, fixed stencils, WENO, spectral and generic models) returns
 * DDD_ERR_UNSUPPORTED with the reason in ddd_last_error(): there is no fallback here,
 * integrate such models one by one.
 *
 * Forcing: everything that is not a weight -- the forcing tables included -- is taken
 * from models[0] AT CALL TIME.  models[0] must therefore outlive the population, and its
 * forcing (ddd_set_forcing with >= batch rows) is the forcing of EVERY replica; the other
 * models' forcing is not looked at.  ddd_population_create synchronises the device (the
 * copies), so a caller that builds a population per call waits on the host once per call.
 *
 * The integrate entry points take the arguments of their solo twins (same checks, same
 * max_attempts default) with replica-major outputs:
 *   adaptive: y_out [R][n_times][batch][N] float64, nfev and status [R][batch]
 *   fixed:    y_out [R][n_steps / save_every][batch][N] float32
 * y0 [batch][N] and `times` are shared by the replicas.  Both end a chained region of
 * models[0] (ddd_stream_fork) and only enqueue on `stream`; `times` travels through
 * models[0]'s page-locked ring as in ddd_integrate_adaptive_f64.  ddd_population_destroy
 * frees the weight copies at once: synchronise `stream` (or order the call behind its
 * work) first. */
typedef struct ddd_population ddd_population;
DDD_API int ddd_population_create(ddd_model* const* models, int replicas, ddd_population** out);
DDD_API int ddd_population_destroy(ddd_population* population);
DDD_API int ddd_population_integrate_adaptive_f64(ddd_population* population,
    const double* times, int n_times, double rtol, double atol, double max_step,
    long long max_attempts, const double* y0, double* y_out, int32_t* nfev, int32_t* status,
    int batch, void* stream);
DDD_API int ddd_population_integrate_fixed(ddd_population* population, int scheme, double t0,
    double dt, int n_steps, int save_every, const float* y0, float* y_out, int batch,
    void* stream);

/* A population kept across calls, whose weights arrive from the device (for instance
 * ddd_train_population_run's [R][n_weights] array): create it once with
 * ddd_population_create_replicated, then ddd_population_load_weights before each rollout.
 * No model handle per replica, no packing on the host, no synchronisation per call. */

/* A population of `replicas` copies of `model`'s packed weights.  Same checks and plans as
 * ddd_population_create on `replicas` models of model's architecture; `model` plays models[0]
 * (launch parameters, forcing, projection tables) and must outlive the population. */
DDD_API int ddd_population_create_replicated(ddd_model* model, int replicas, ddd_population** out);

/* Packs `count` weight vectors in ddd_model_create's layout, DEVICE [count][n_weights], into
 * replicas first_replica .. first_replica + count - 1, on `stream`: afterwards those replicas
 * hold bit for bit what ddd_model_create + ddd_population_create would have given them.
 * Enqueue only: no allocation, no copy to or from the host, no synchronisation.  Ordered
 * against rollouts by stream order; loading while a rollout of this population runs on
 * another stream is the caller's error.  Works on populations from either constructor.
 * DDD_ERR_INVALID_ARGUMENT: NULL pointers, a range outside the population, an n_weights
 * that is not the model's. */
DDD_API int ddd_population_load_weights(ddd_population* population, const float* weights,
                                        size_t n_weights, int first_replica, int count,
                                        void* stream);

/* ---- differentiable evaluation --------------------------------------------
 * Replaces: tf.gradients through model.predict_result (model.py:664-697), the
 * building block of the reference's differentiable time integration
 * (predict_time_evolution, model.py:643-661).  One model evaluation
 * [batch][N] -> predictions [batch][N][H] (result_stack order, as
 * ddd_train_args.predictions: the space derivatives, then the equation of
 * motion, no forcing) and its vector-Jacobian product: for a cotangent
 * c [batch][N][H], grad_y = c^T d predictions / d y and grad_weights =
 * c^T d predictions / d weights (summed over the batch).  Stateless like the
 * training ABI: the weights are a device vector in the ddd_model_create layout.
 * Supports exactly the configurations ddd_train_loss_grad supports; the others
 * return DDD_ERR_UNSUPPORTED before any device work.
 * Deterministic: grad_y is per sample (a gather, no cross-sample sum);
 * grad_weights is summed over the batch in fixed-order partial slabs, no
 * atomics, so equal inputs give bit-identical outputs. */
typedef struct ddd_vjp_args {
  int32_t struct_size;   /* = sizeof(ddd_vjp_args), checked */
  int32_t batch;         /* rows of y */
  const float* weights;  /* conv weights (ddd_model_create layout, as ddd_train_args) */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y;        /* [batch][N] */
  const float* cotangent; /* [batch][N][H], or NULL: forward only */
  float* predictions;    /* out [batch][N][H] or NULL */
  float* grad_y;         /* out [batch][N] or NULL */
  float* grad_weights;   /* out, layout of `weights`, or NULL */
  void* workspace;       /* ddd_vjp_workspace_bytes(cfg, batch) bytes */
  size_t workspace_bytes;
} ddd_vjp_args;

/* Bytes of the caller-allocated workspace of ddd_result_vjp for `batch` samples
 * (partial weight-gradient slabs and per-workgroup scratch); 0 on error. */
DDD_API size_t ddd_vjp_workspace_bytes(const ddd_config* cfg, int batch);
/* Without a cotangent: the predictions only (predictions must then be non-NULL,
 * grad_y and grad_weights NULL).  With one: at least one of grad_y and
 * grad_weights, and the predictions too when non-NULL.  The forward pass is
 * recomputed inside the call; nothing is kept between calls. */
DDD_API int ddd_result_vjp(const ddd_config* cfg, const ddd_vjp_args* args, void* stream);

/* ---- tangent-linear model ---------------------------------------------------
 * Forward mode beside ddd_result_vjp's reverse mode: the Jacobian of one model
 * evaluation applied to vectors, and state perturbations carried along a
 * rollout (stability of the linearised scheme, Lyapunov exponents).  Stateless,
 * the weights a device vector in the ddd_model_create layout; exactly the
 * configurations ddd_result_vjp supports, the others return DDD_ERR_UNSUPPORTED
 * before any device work.  No forcing: the forcing term depends neither on the
 * state nor on the weights.  Deterministic: every output is per sample, no
 * atomics, no cross-sample sum, so equal inputs give bit-identical outputs. */
#define DDD_MAX_TANGENTS 32

typedef struct ddd_jvp_args {
  int32_t struct_size;   /* = sizeof(ddd_jvp_args), checked */
  int32_t batch;         /* rows of y */
  int32_t tangents;      /* M, tangents per sample, in [1, DDD_MAX_TANGENTS] */
  int32_t reserved;      /* 0 */
  const float* weights;  /* conv weights (ddd_model_create layout, as ddd_train_args) */
  const float* nullspace; /* as ddd_train_args */
  const float* bias;     /* as ddd_train_args */
  const float* y;        /* [batch][N] */
  const float* tangent_y; /* [batch][M][N] directions of the state, or NULL */
  const float* tangent_weights; /* [M][n_weights] directions of the weights, shared by the
                          * batch, or NULL */
  float* predictions;    /* out [batch][N][H] or NULL (bit for bit ddd_result_vjp's) */
  float* tangents_out;   /* out [batch][M][N][H] */
  void* workspace;       /* ddd_jvp_workspace_bytes(cfg, batch, tangents) bytes */
  size_t workspace_bytes;
} ddd_jvp_args;

/* Bytes of the caller-allocated workspace of ddd_result_jvp (per-workgroup scratch);
 * 0 on error. */
DDD_API size_t ddd_jvp_workspace_bytes(const ddd_config* cfg, int batch, int tangents);
/* tangents_out[b][j] = d predictions / d y (y[b]) tangent_y[b][j]
 *                    + d predictions / d weights (y[b]) tangent_weights[j].
 * At least one of tangent_y and tangent_weights; with both, the sum of the two
 * contributions.  The space-derivative channels of model_target 'time_derivative'
 * are zero, and so is their tangent.  The forward pass runs once per sample. */
DDD_API int ddd_result_jvp(const ddd_config* cfg, const ddd_jvp_args* args, void* stream);

typedef struct ddd_tangent_rollout_args {
  int32_t struct_size;   /* = sizeof(ddd_tangent_rollout_args), checked */
  int32_t batch;         /* rows of y0 */
  int32_t tangents;      /* M, tangents per sample, in [1, DDD_MAX_TANGENTS] */
  int32_t num_steps;     /* >= 1 */
  double dt;             /* step size */
  const float* weights;  /* as ddd_jvp_args */
  const float* nullspace;
  const float* bias;
  const float* y0;       /* [batch][N] */
  const float* tangents0; /* [batch][M][N] state tangents at y0 */
  float* state_out;      /* out [batch][N] the state after num_steps steps */
  float* tangents_out;   /* out [batch][M][N] the tangents after num_steps steps */
  void* workspace;       /* ddd_tangent_rollout_workspace_bytes(cfg, batch, tangents) bytes */
  size_t workspace_bytes;
} ddd_tangent_rollout_args;

DDD_API size_t ddd_tangent_rollout_workspace_bytes(const ddd_config* cfg, int batch,
                                                   int tangents);
/* num_steps explicit-midpoint steps of the state and of its M tangents in one launch:
 *   k1 = f(y), dk1 = J(y) t;  y_m = y + dt/2 k1, t_m = t + dt/2 dk1;
 *   k2 = f(y_m), dk2 = J(y_m) t_m;  y += dt k2, t += dt dk2.
 * State tangents only, and unforced (like model.differentiable_time_evolution).
 * Nothing per step is kept. */
DDD_API int ddd_tangent_rollout(const ddd_config* cfg, const ddd_tangent_rollout_args* args,
                                void* stream);

/* ---- introspection -------------------------------------------------------*/
DDD_API int ddd_set_kernel(ddd_model* model, int kernel_kind);
/* "mfma_f32_r64", "mfma_f32_r64w32", "mfma_f32_r64w16" (small ensembles: every 64-row group
 * on two / four wavefronts), "mfma_f32_r64h16" (nets of up to 16 filters on 16-channel tiles,
 * persistent integrators), "mfma_f32_r256", "generic", "valu_f32_lean" (fixed
 * stencils / one-layer nets, persistent launch: lane == grid point, no matrix work),
 * "valu_f32_weno" (WENO5 + Godunov flux, integrate.py:124-140: one wavefront per sample),
 * "stream_fixed" (fixed stencils, one launch per substep or step) or "spectral_f64":
 * the kernel family and workgroup geometry of the most recent launch on this
 * handle (the automatic choice depends on the batch size and launch mode). */
DDD_API const char* ddd_kernel_name(const ddd_model* model);
/* Algorithmic multiply-adds per grid point per right-hand-side evaluation
 * (SURVEY.md section 8(d)); 2x this is the FLOP count used for the roofline. */
DDD_API int64_t ddd_fma_per_point(const ddd_model* model);
/* Number of right-hand-side evaluations per step of a scheme. */
DDD_API int ddd_scheme_stages(int scheme);
/* Runs tiny MFMA probes on the current device and checks the operand/result
 * register layouts the kernels assume; 0 = layouts as assumed. */
DDD_API int ddd_selftest_mfma_layout(void);
DDD_API int ddd_abi_version(void);
DDD_API const char* ddd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DDD1D_H_ */
