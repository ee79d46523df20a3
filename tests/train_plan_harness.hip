// csrc/train_plan.h without a device: every number the planner sets, for a fixed table of
// cases, one JSON object per line (tests/test_cpu_train_plan.py compares them with
// tests/golden/train_plans.json).  A stand-alone program: it calls no HIP function, so it
// runs where there is no GPU, and a host-sanitizer build of it checks the planner.
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../data-driven-discretization-1d_amd/csrc/train_plan.h"

// capi_common.h's definitions live in capi.hip, next to the model code; these stand in
// for them (every case of the table is a configuration the common checks admit).
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
int common_config_checks(const ddd_config* cfg) {
  if (cfg == nullptr || cfg->struct_size != (int32_t)sizeof(ddd_config))
    return fail(DDD_ERR_INVALID_ARGUMENT, "cfg");
  return DDD_OK;
}
bool is_conservative(int eq) { return eq % 2 == 1; }   // (of the equations training admits)
bool is_forced_family(int eq) { return eq <= DDD_EQ_BURGERS_CONSERVATIVE; }
}  // namespace capi
}  // namespace ddd

using namespace ddd::train;

namespace {

// What one plan leaves: the launch, the slab and LDS layout in p, the through-time offsets
// (-1: the plan has none) and the rollout-run tail
struct Row {
  int rc = 0, blocks = 0;
  size_t lds_bytes = 0, ws_bytes = 0;
  TrainParams p;
  int HT = -1, st_off = -1, gi_off = -1;
  long grad_buf = -1, partials = -1, decisions = -1;
};

// ---- the seven plans ---------------------------------------------------------
Row training(const ddd_config& cfg, int batch) {
  Row r;
  LaunchPlan lp{};
  r.rc = plan_training(&cfg, batch, &r.p, &lp);
  r.blocks = lp.blocks, r.lds_bytes = lp.lds_bytes, r.ws_bytes = lp.ws_bytes;
  return r;
}

Row unrolled(const ddd_config& cfg, int batch, int T) {
  Row r;
  UnrolledParams q;
  LaunchPlan lp{};
  r.rc = plan_unrolled(&cfg, batch, T, &q, &lp);
  r.blocks = lp.blocks, r.lds_bytes = lp.lds_bytes, r.ws_bytes = lp.ws_bytes;
  r.p = q.t, r.HT = q.HT, r.st_off = q.st_off, r.gi_off = q.gi_off;
  return r;
}

Row rollout(const ddd_config& cfg, int batch, int T) {
  Row r;
  RolloutParams q;
  LaunchPlan lp{};
  r.rc = plan_rollout(&cfg, batch, T, &q, &lp);
  r.blocks = lp.blocks, r.lds_bytes = lp.lds_bytes, r.ws_bytes = lp.ws_bytes;
  r.p = q.t, r.st_off = q.st_off, r.gi_off = q.gi_off;
  return r;
}

Row population(const ddd_config& cfg, int batch, int T, int R, const char* who) {
  Row r;
  RunParams run;
  LaunchPlan lp{};
  r.rc = plan_population(&cfg, batch, T, R, &run, &lp, who);
  r.blocks = run.blocks, r.lds_bytes = run.lds_bytes, r.ws_bytes = lp.ws_bytes;
  r.p = run.q.t, r.HT = run.q.HT, r.st_off = run.q.st_off, r.gi_off = run.q.gi_off;
  return r;
}

Row run(const ddd_config& cfg, int batch, int T) {
  return population(cfg, batch, T, 1, "training run");
}

Row metrics(const ddd_config& cfg, int batch, int T, int R) {
  Row r;
  MetricsParams m;
  LaunchPlan lp{};
  r.rc = plan_metrics(&cfg, batch, T, R, &m, &lp);
  r.blocks = m.blocks, r.lds_bytes = m.lds_bytes, r.ws_bytes = lp.ws_bytes;
  r.p = m.q.t, r.HT = m.q.HT, r.st_off = m.q.st_off, r.gi_off = m.q.gi_off;
  return r;
}

Row rollout_run(const ddd_config& cfg, int batch, int T, int R) {
  Row r;
  RolloutRunParams rr;
  LaunchPlan lp{};
  r.rc = plan_rollout_run(&cfg, batch, T, R, &rr, &lp);
  r.blocks = rr.blocks, r.lds_bytes = rr.lds_bytes, r.ws_bytes = lp.ws_bytes;
  r.p = rr.q.t, r.st_off = rr.q.st_off, r.gi_off = rr.q.gi_off;
  r.grad_buf = (long)lp.grad_buf, r.partials = (long)lp.partials;
  r.decisions = (long)lp.decisions;
  return r;
}
// ---- end of the seven plans --------------------------------------------------

void print_ints(const char* name, const int* v, int n) {
  std::printf(", \"%s\": [", name);
  for (int i = 0; i < n; ++i) std::printf("%s%d", i ? ", " : "", v[i]);
  std::printf("]");
}

void print_row(const char* name, const char* plan, const ddd_config& cfg, int batch, int T,
               int R, const Row& r) {
  const TrainParams& p = r.p;
  std::printf("{\"case\": \"%s\", \"plan\": \"%s\", \"batch\": %d, \"T\": %d, \"R\": %d", name,
              plan, batch, T, R);
  std::printf(", \"cfg\": {\"equation\": %d, \"num_points\": %d, \"num_derivatives\": %d, "
              "\"stencil_size\": %d, \"model_target\": %d, \"num_layers\": %d, "
              "\"filter_size\": %d, \"kernel_size\": %d, \"polynomial_accuracy_order\": %d",
              cfg.equation, cfg.num_points, cfg.num_derivatives, cfg.stencil_size,
              cfg.model_target, cfg.num_layers, cfg.filter_size, cfg.kernel_size,
              cfg.polynomial_accuracy_order);
  print_ints("input_sizes", cfg.input_sizes, DDD_MAX_DERIVATIVES);
  std::printf("}, \"rc\": %d, \"blocks\": %d, \"lds_bytes\": %zu, \"ws_bytes\": %zu", r.rc,
              r.blocks, r.lds_bytes, r.ws_bytes);
  std::printf(", \"n_weights\": %d, \"n_slab\": %d, \"slab_stride\": %zu, \"st_off\": %d, "
              "\"gi_off\": %d, \"HT\": %d, \"mfma\": %d, \"wl_floats\": %d, \"cmax\": %d, "
              "\"C_out\": %d", p.n_weights, p.n_slab, p.slab_stride, r.st_off, r.gi_off, r.HT,
              p.mfma, p.wl_floats, p.cmax, p.C_out);
  print_ints("wl_off", p.wl_off, p.L);
  print_ints("w_off", p.w_off, p.L);
  print_ints("z_off", p.z_off, p.L);
  print_ints("cin", p.cin, p.L);
  print_ints("cout", p.cout, p.L);
  print_ints("in_start", p.in_start, ddd::kMaxDerivs);
  print_ints("in_size", p.in_size, ddd::kMaxDerivs);
  print_ints("ns_off", p.ns_off, ddd::kMaxDerivs);
  std::printf(", \"grad_buf\": %ld, \"partials\": %ld, \"decisions\": %ld}\n", r.grad_buf,
              r.partials, r.decisions);
}

// The configuration of tests/test_cpu_training.py's _config(): Burgers, 32 points, three
// layers of 32 filters and 5 taps, target space_derivatives
ddd_config default_config() {
  ddd_config cfg{};
  cfg.struct_size = (int32_t)sizeof(cfg);
  cfg.equation = DDD_EQ_BURGERS;
  cfg.num_points = 32;
  cfg.num_derivatives = 2;
  cfg.derivative_orders[0] = 1;
  cfg.derivative_orders[1] = 2;
  cfg.dx = 1.0 / 32;
  cfg.period = 1.0;
  cfg.standard_deviation = 1.0;
  cfg.stencil_size = 6;
  cfg.model_target = DDD_TARGET_SPACE_DERIVATIVES;
  cfg.num_layers = 3;
  cfg.filter_size = 32;
  cfg.kernel_size = 5;
  return cfg;
}

ddd_config ks_config(int target, int order) {
  ddd_config cfg = default_config();
  cfg.equation = DDD_EQ_KS;
  cfg.num_derivatives = 3;
  cfg.derivative_orders[2] = 4;
  cfg.stencil_size = 7;
  cfg.model_target = target;
  cfg.polynomial_accuracy_order = order;
  if (order > 0) cfg.input_sizes[0] = 5, cfg.input_sizes[1] = 4, cfg.input_sizes[2] = 2;
  return cfg;
}

ddd_config big_config(int layers, int taps) {
  ddd_config cfg = default_config();
  cfg.num_points = 256;
  cfg.dx = 1.0 / 256;
  cfg.num_layers = layers;
  cfg.kernel_size = taps;
  return cfg;
}

// One row per plan: the unrolled kernel at Tu steps, the rollout kernels at Tr, the run,
// population and metrics plans at Tm, the replicated ones with R replicas
void all_plans(const char* name, const ddd_config& cfg, int batch, int Tu, int Tr, int Tm,
               int R) {
  print_row(name, "training", cfg, batch, 0, 1, training(cfg, batch));
  print_row(name, "unrolled", cfg, batch, Tu, 1, unrolled(cfg, batch, Tu));
  print_row(name, "rollout", cfg, batch, Tr, 1, rollout(cfg, batch, Tr));
  print_row(name, "run", cfg, batch, Tm, 1, run(cfg, batch, Tm));
  print_row(name, "population", cfg, batch, Tm, R, population(cfg, batch, Tm, R,
                                                              "training population"));
  print_row(name, "metrics", cfg, batch, Tm, R, metrics(cfg, batch, Tm, R));
  print_row(name, "rollout_run", cfg, batch, Tr, R, rollout_run(cfg, batch, Tr, R));
}

// ... and the plans that depend on them again at other steps and replicas
void through_time(const char* name, const ddd_config& cfg, int batch, int Tu, int Tr, int Tm,
                  int R) {
  print_row(name, "unrolled", cfg, batch, Tu, 1, unrolled(cfg, batch, Tu));
  print_row(name, "rollout", cfg, batch, Tr, 1, rollout(cfg, batch, Tr));
  print_row(name, "run", cfg, batch, Tm, 1, run(cfg, batch, Tm));
  print_row(name, "population", cfg, batch, Tm, R, population(cfg, batch, Tm, R,
                                                              "training population"));
  print_row(name, "metrics", cfg, batch, Tm, R, metrics(cfg, batch, Tm, R));
  print_row(name, "rollout_run", cfg, batch, Tr, R, rollout_run(cfg, batch, Tr, R));
}

}  // namespace

int main() {
  const ddd_config def = default_config();
  // staged kernels; every value of T and R the cases ask for
  all_plans("default", def, 4, 1, 1, 0, 1);
  through_time("default", def, 4, 8, 9, 2, 2);
  through_time("default", def, 4, 8, 256, 2, 64);
  // not a multiple of 32: VALU
  ddd_config cfg = def;
  cfg.num_points = 40;
  cfg.dx = 1.0 / 40;
  all_plans("points40", cfg, 4, 8, 9, 2, 2);
  // no 32 -> 32 layer: nothing to stage
  cfg = def;
  cfg.filter_size = 16;
  all_plans("filters16", cfg, 4, 8, 9, 2, 2);
  // the staged kernels fit for one evaluation and not next to the two through-time rows
  all_plans("big6x5", big_config(6, 5), 4, 1, 1, 0, 1);
  through_time("big6x5", big_config(6, 5), 4, 8, 9, 2, 2);
  // nothing fits anywhere
  all_plans("big8x7", big_config(8, 7), 4, 1, 1, 0, 1);
  through_time("big8x7", big_config(8, 7), 4, 8, 9, 2, 2);
  all_plans("ks_projected", ks_config(DDD_TARGET_COEFFICIENTS, 1), 4, 8, 9, 2, 2);
  all_plans("ks_order0", ks_config(DDD_TARGET_COEFFICIENTS, 0), 4, 1, 1, 0, 1);
  all_plans("ks_space_derivatives", ks_config(DDD_TARGET_SPACE_DERIVATIVES, 0), 4, 8, 9, 2, 2);
  // below, at and above the 512 workgroups
  all_plans("batch1", def, 1, 1, 1, 0, 1);
  all_plans("batch512", def, 512, 8, 9, 2, 2);
  all_plans("batch4096", def, 4096, 8, 9, 2, 64);
  return 0;
}
