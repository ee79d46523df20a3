// TEST INFRASTRUCTURE ONLY (CPU test tier; never part of the product).
//
// Drives the PRODUCT header csrc/rk23.h -- the per-sample RK23 controller, the
// per-grid-point formulas and rk23::solve_uniform, the very loop the generic
// adaptive kernel runs (f0, the initial-step probe, stages 2 / 3 / FSAL, dense
// output, attempt limit, NaN rows) -- on the CPU, over a right-hand side
// supplied by the caller (a Python callback in tests/test_cpu_rk23_source.py).
// Only the backend below is the harness's own: one thread that owns every
// point.  What it proves without a GPU: the device source itself, not a twin
// of it, reproduces scipy.integrate.solve_ivp(method='RK23') (the reference's
// integrator, pde_superresolution/integrate.py:154-155).  (The WENO and
// spectral kernels keep hand copies of that loop, and rhs_adaptive.h shares the
// controller and the formulas, not the loop: for those the GPU tier's parity
// tests stand.)
#define DDD_RK23_HOST 1
#include "../data-driven-discretization-1d_amd/csrc/rk23.h"

#include <cmath>
#include <limits>
#include <vector>

using ddd::rk23::Control;
namespace rk = ddd::rk23;

// KT: float (TF-graph models, generic and WENO kernels) or double (spectral solver)
template <typename T>
struct HostBackend {
  typedef T KT;
  void (*fun)(double, const double*, KT*, void*);
  void* user;
  int n;
  double* u;
  double* y_out;            // [n_times][n]
  double *y, *y_new;
  KT *k0, *k1, *k2, *f;

  template <typename F>
  void each(F fn) const { for (int i = 0; i < n; ++i) fn(i); }
  void input(int i, double v) const { u[i] = v; }
  void eval(double t) const { fun(t, u, f, user); }
  double sum(double part) const { return part; }
  void store(int row, int i, double v) const { y_out[(long)row * n + i] = v; }
  void end_phase() const {}
};

template <typename KT>
static int solve(void (*fun)(double, const double*, KT*, void*), void* user, int n,
                 const double* times, int n_times, double rtol, double atol, double max_step,
                 long long max_attempts, const double* y0, double* y_out, int* nfev_out) {
  std::vector<double> y(y0, y0 + n), y_new(y0, y0 + n), u(n);
  std::vector<KT> k0(n), k1(n), k2(n), f(n);
  HostBackend<KT> b{fun, user, n, u.data(), y_out,
                    y.data(), y_new.data(), k0.data(), k1.data(), k2.data(), f.data()};
  if (max_attempts <= 0) max_attempts = std::numeric_limits<long long>::max();   // no limit
  Control c;
  rk::solve_uniform(b, c, times, n_times, rtol, atol, max_step, max_attempts,
                    std::sqrt((double)n));
  *nfev_out = c.nfev;
  return c.status;
}

extern "C" {
int rk23_host_solve_f32(void (*fun)(double, const double*, float*, void*), void* user, int n,
                        const double* times, int n_times, double rtol, double atol,
                        double max_step, long long max_attempts, const double* y0,
                        double* y_out, int* nfev) {
  return solve<float>(fun, user, n, times, n_times, rtol, atol, max_step, max_attempts, y0, y_out,
                      nfev);
}
int rk23_host_solve_f64(void (*fun)(double, const double*, double*, void*), void* user, int n,
                        const double* times, int n_times, double rtol, double atol,
                        double max_step, long long max_attempts, const double* y0,
                        double* y_out, int* nfev) {
  return solve<double>(fun, user, n, times, n_times, rtol, atol, max_step, max_attempts, y0,
                       y_out, nfev);
}
}
