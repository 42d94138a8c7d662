// bann_hmc.hip — the packed HMC driver of include/bann.h: a trajectory's start (traj_prepare),
// its launch sequence (traj_run, the one place that holds it), graph replay, bann_hmc_step,
// the sequential driver's hmc_step_tail, bann_hmc_step_joint, trajectory recording, launch
// timing and the leapfrog session.
//
// Host-side counterpart of the reference's hmc_step (branch_sampler.rs:1192-1299),
// hmc_step_joint (1070-1178) and its step-size rules.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "ctx_internal.h"

// random step sizes (branch_sampler.rs:654-681): U(0,1) * P^(-1/4) * c, drawn on
// the host; uniform (706-732) and Izmailov (ridge_ard.rs:70-117, ridge_base.rs:
// 83-114, lasso_ard.rs:77-117, lasso_base.rs:83-114, std_normal_branch.rs:83-114)
// are formed on the device from step_bases (bann_branch.hip).
static void host_random_step_sizes(const BranchHost& h, float c, std::mt19937_64& rng, std::vector<float>& eps) {
  eps.assign(h.P, c);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  const float f = powf((float)h.P, -0.25f) * c;
  for (auto& e : eps) e = U(rng) * f;
}

// StdScaled step sizes (dispatched at branch_sampler.rs:1213) for the Base priors:
// ridge_base.rs:52-82, lasso_base.rs:53-82, std_normal_branch.rs:51-80 -- in f32 as the
// reference: weights c * (1 / lambda_l).sqrt() (host scalar), biases
// c * (1 / sqrt(lambda_b)) (the lasso form 1 * c * (1 / sqrt) rounds identically).
// The ARD priors return empty vectors (ridge_ard.rs:56-68, lasso_ard.rs:62-74): refused.
static bool host_std_scaled_step_sizes(const BranchHost& h, float c, std::vector<float>& eps) {
  if (h.prior == BANN_RIDGE_ARD || h.prior == BANN_LASSO_ARD) return false;
  const BranchDev& d = h.dev;
  eps.assign(h.P, 0.f);
  for (int l = 0; l < h.L; ++l) {
    const volatile float inv = 1.f / h.prec[l];
    const float e = c * sqrtf(inv);
    const int cnt = d.win[l] * d.widths[l];
    for (int k = 0; k < cnt; ++k) eps[d.woff[l] + k] = e;
  }
  for (int l = 0; l < h.L - 1; ++l) {
    const volatile float rs = 1.f / sqrtf(h.prec[h.L + l]);
    const float e = c * rs;
    for (int k = 0; k < d.widths[l]; ++k) eps[d.boff[l] + k] = e;
  }
  return true;
}

int ensure_htrace(bann_ctx* ctx, int32_t L) {
  if (L + 1 <= ctx->htrace_cap) return BANN_OK;
  const int32_t cap = std::max({L + 1, 2 * ctx->htrace_cap, 129});  // grow geometrically: no realloc per trajectory
  dfree(ctx->d_htrace);
  ctx->d_htrace = nullptr;
  CK(dalloc(&ctx->d_htrace, (int64_t)ctx->br.size() * cap));
  ctx->htrace_cap = cap;
  refresh_state(ctx);
  return BANN_OK;
}

// the -H trace of a trajectory of L steps: room for it, and the by-value state that goes with it
static int trace_setup(bann_ctx* ctx, int32_t L, float max_dh) {
  const int rc = ensure_htrace(ctx, L);
  if (rc) return rc;
  ctx->st.max_dh = max_dh;
  ctx->st.lint = ctx->htrace_cap - 1;
  return BANN_OK;
}

// every entry NaN: an early rejection leaves the later ones unwritten
static hipError_t trace_clear(bann_ctx* ctx) {
  return hipMemsetAsync(ctx->d_htrace, 0xFF, ctx->br.size() * ctx->htrace_cap * sizeof(double), ctx->stream);
}

int traj_prepare(bann_ctx* ctx, const Plan& p, int32_t L, float max_dh, int32_t step_mode, float factor,
                 const float* eps, const float* momentum, uint64_t seed, const float* u) {
  int rc = trace_setup(ctx, L, max_dh);
  if (rc) return rc;
  std::mt19937_64 rng(seed ^ 0x5DEECE66Dull);
  std::vector<float> e;
  int64_t off = 0;
  const bool device_eps = step_mode == BANN_STEP_UNIFORM || step_mode == BANN_STEP_IZMAILOV;
  if (device_eps) {
    launch_step_sizes(ctx->st, ctx->d_stepbase, p.d_all, (int32_t)p.all.size(), p.max_p,
                      step_mode == BANN_STEP_UNIFORM ? 0 : 1, factor, L, ctx->stream);
    CK(hipGetLastError());
  }
  for (int32_t b : p.all) {
    const BranchHost& h = ctx->br[b];
    if (device_eps) {
      // formed on the device above
    } else if (step_mode == BANN_STEP_INJECTED) {
      if (!eps) return fail(ctx, BANN_E_ARG, "injected step sizes need eps");
      CK(hipMemcpyAsync(ctx->d_eps + h.dev.p_off, eps + off, h.P * sizeof(float), hipMemcpyHostToDevice,
                        ctx->stream));
    } else if (step_mode == BANN_STEP_STD_SCALED) {
      if (!host_std_scaled_step_sizes(h, factor, e))
        return fail(ctx, BANN_E_ARG,
                    "StdScaled step sizes are empty for the ARD priors in the reference (ridge_ard.rs:56-68, "
                    "lasso_ard.rs:62-74; hmc_step would index-panic): use Izmailov, uniform or random");
      CK(hipMemcpyAsync(ctx->d_eps + h.dev.p_off, e.data(), h.P * sizeof(float), hipMemcpyHostToDevice,
                        ctx->stream));
      CK(hipStreamSynchronize(ctx->stream));  // e is reused for the next branch
    } else {
      if (step_mode != BANN_STEP_RANDOM) return fail(ctx, BANN_E_ARG, "unknown step size mode");
      host_random_step_sizes(h, factor, rng, e);
      CK(hipMemcpyAsync(ctx->d_eps + h.dev.p_off, e.data(), h.P * sizeof(float), hipMemcpyHostToDevice,
                        ctx->stream));
    }
    if (momentum)
      CK(hipMemcpyAsync(ctx->d_mom + h.dev.p_off, momentum + off, h.P * sizeof(float), hipMemcpyHostToDevice,
                        ctx->stream));
    off += h.P;
  }
  if (!momentum) {
    launch_sample_momentum(ctx->st, p.d_all, (int32_t)p.all.size(), p.max_p, seed, ctx->stream);
    CK(hipGetLastError());
  }
  if (u) {  // injected acceptance uniforms (parity runs; the sequential driver's host draws)
    // staged in pinned memory that outlives the copy: no host wait here (the stage is
    // reused once the previous call's copy has completed)
    if (!ctx->h_u_stage) {
      CK(hipHostMalloc((void**)&ctx->h_u_stage, ctx->br.size() * sizeof(float), hipHostMallocDefault));
      CK(hipEventCreateWithFlags(&ctx->ev_u, hipEventDisableTiming));
      std::fill(ctx->h_u_stage, ctx->h_u_stage + ctx->br.size(), 0.f);
    }
    if (ctx->u_ev_pending) CK(hipEventSynchronize(ctx->ev_u));
    for (size_t i = 0; i < p.all.size(); ++i) ctx->h_u_stage[p.all[i]] = u[i];
    CK(hipMemcpyAsync(ctx->d_u, ctx->h_u_stage, ctx->br.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    CK(hipEventRecord(ctx->ev_u, ctx->stream));
    ctx->u_ev_pending = true;
  } else {  // u ~ U(0,1) per branch (branch_sampler.rs:546-548) on the device
    launch_uniforms(ctx->st, p.d_all, (int32_t)p.all.size(), seed, ctx->stream);
  }
  CK(trace_clear(ctx));
  // device-only trajectory start (leapfrog sessions): no host round trip; host
  // vectors (random / injected step sizes, injected momenta) must outlive their copies
  if (momentum || !device_eps) CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// per-branch outputs of a finished bann_hmc_step (the stream has drained)
static int hmc_outputs(bann_ctx* ctx, const int32_t* branches, int32_t nb, int32_t L, int32_t* status_out,
                       double* h_trace_out, int32_t* uturn_out, double* log_density_out) {
  const int stride = ctx->htrace_cap;
  for (int i = 0; i < nb; ++i) {
    const int b = branches[i];
    if (status_out) CK(hipMemcpy(status_out + i, ctx->d_status + b, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (uturn_out) CK(hipMemcpy(uturn_out + i, ctx->d_uturn + b, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (log_density_out) CK(hipMemcpy(log_density_out + i, ctx->d_ld + b, sizeof(double), hipMemcpyDeviceToHost));
    if (h_trace_out)
      CK(hipMemcpy(h_trace_out + (int64_t)i * (L + 1), ctx->d_htrace + (int64_t)b * stride, (L + 1) * sizeof(double),
                   hipMemcpyDeviceToHost));
  }
  return BANN_OK;
}

// ---- graph replay of a trajectory's launch sequence (bann_hmc_step) ----
// The sequential driver runs one small trajectory after another (one branch,
// L steps of gradient + update launches): the host's launch overhead, not the
// GPU, paces it.  The sequence of a plan shape is captured once into a HIP
// graph and replayed; the plan's device arrays live in the context's scratch
// buffers (fixed addresses), so one graph serves every branch of the same shape.
// The key holds everything the captured kernel arguments depend on and that can change
// within a context: graphs are cached per context and the BANN_* switches (bann_ctx::opt)
// are fixed for its life, so none of them is a field; wide_bf16 is one, being settable.
static std::string traj_graph_key(const bann_ctx* ctx, const Plan& p, int32_t L) {
  std::string k;
  auto put = [&](int64_t v) { k.append(reinterpret_cast<const char*>(&v), sizeof(v)); };
  put(L);
  put(ctx->wide_bf16);
  put((int64_t)p.all.size());
  put(p.n_small);
  put(p.n_large);
  put(p.max_p);
  put(p.fuse_update);
  put((int64_t)p.fold.size());
  put((int64_t)(intptr_t)p.d_all);
  put((int64_t)(intptr_t)p.d_fold);
  put((int64_t)(intptr_t)p.d_gx);
  put((int64_t)(intptr_t)p.d_gxpre);
  for (const auto& g : p.groups) {
    put(g.kind), put(g.L), put(g.act), put(g.nw), put(g.cpw), put(g.full), put(g.head);  // cpw, head: fxl's kernel
    put((int64_t)g.items.size());
    put((int64_t)(intptr_t)g.d_items);
  }
  for (const auto& g : p.gxg) {
    put(g.first), put(g.count), put(g.max_splits);
    for (const auto& ph : g.phases) put(ph.ph), put(ph.l), put(ph.total), put(ph.pre_off);
  }
  k.append(reinterpret_cast<const char*>(&ctx->st), sizeof(DevState));  // the kernels' by-value state
  return k;
}

void clear_graphs(bann_ctx* ctx) {
  for (auto& e : ctx->graphs) (void)hipGraphExecDestroy(e.second);
  ctx->graphs.clear();
}

// the trace, the uniforms' stage, the captured graphs, the timing events and the session's plan
void hmc_release(bann_ctx* ctx) {
  free_plan(ctx->lf);
  clear_graphs(ctx);
  for (hipEvent_t e : ctx->tm_pool) (void)hipEventDestroy(e);
  ctx->tm_pool.clear();
  ctx->tm_marks.clear();
  if (ctx->u_ev_pending && ctx->ev_u) (void)hipEventSynchronize(ctx->ev_u);  // the copy has read the stage
  ctx->u_ev_pending = false;
  if (ctx->h_u_stage) (void)hipHostFree(ctx->h_u_stage);
  if (ctx->ev_u) (void)hipEventDestroy(ctx->ev_u);
  ctx->h_u_stage = nullptr;
  ctx->ev_u = nullptr;
  dfree_all(ctx->d_htrace);
  ctx->htrace_cap = 0;
}

// ---- trajectory recording (mcmc_cfg.trajectories, trajectory.rs) ----
// room for L steps of every listed branch: params[k-1] = theta_k (after the k-th position
// step), ldg[k-1] = the log-density gradient there; the joint Trajectory (branch_sampler.rs:
// 1126-1135) also keeps the precisions and appends their gradient to ldg's rows
static void rec_begin(bann_ctx* ctx, const int32_t* branches, int32_t nb, int32_t L, bool joint) {
  ctx->rec.resize(ctx->br.size());
  for (int i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    auto& R = ctx->rec[branches[i]];
    R.q = joint ? h.dev.nq : 0;
    R.params.assign((size_t)L * h.P, 0.f);
    R.prec.assign((size_t)L * R.q, 0.f);
    R.ldg.assign((size_t)L * (h.P + R.q), 0.f);
  }
}

// traj_run's hook of a recorded trajectory, step k: after the gradient launch (theta_k, phi_k),
// after the update launch the gradient it folded
static int rec_step(bann_ctx* ctx, const int32_t* branches, int32_t nb, int k, bool updated) {
  for (int i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    auto& R = ctx->rec[branches[i]];
    float* row = updated ? R.ldg.data() + (size_t)(k - 1) * (h.P + R.q) : R.params.data() + (size_t)(k - 1) * h.P;
    CK(hipMemcpyAsync(row, (updated ? ctx->d_grad : ctx->d_theta) + h.dev.p_off, h.P * sizeof(float),
                      hipMemcpyDeviceToHost, ctx->stream));
    if (R.q)
      CK(hipMemcpyAsync(updated ? row + h.P : R.prec.data() + (size_t)(k - 1) * R.q,
                        (updated ? ctx->d_gphi : ctx->d_phi) + h.dev.q_off, R.q * sizeof(float), hipMemcpyDeviceToHost,
                        ctx->stream));
  }
  return BANN_OK;
}

// the -H trace of every recorded branch after the stream has drained; an early rejection
// leaves the later entries unwritten (NaN) and ends the recorded steps there
// (branch_sampler.rs:1264-1279)
static int rec_finish(bann_ctx* ctx, const int32_t* branches, int32_t nb, int32_t L) {
  const int stride = ctx->htrace_cap;
  for (int i = 0; i < nb; ++i) {
    auto& R = ctx->rec[branches[i]];
    R.h.assign(L + 1, 0.0);
    CK(hipMemcpy(R.h.data(), ctx->d_htrace + (int64_t)branches[i] * stride, (L + 1) * sizeof(double),
                 hipMemcpyDeviceToHost));
    int steps = 0;
    while (steps < L && R.h[steps + 1] == R.h[steps + 1]) ++steps;
    R.steps = steps;
    R.h.resize(steps + 1);
  }
  return BANN_OK;
}

// ---- the launch sequence of a trajectory ----
enum TrajUpdate {  // the update that follows a gradient launch
  UPD_SEPARATE,    // run_update's kernels
  UPD_FUSED,       // in the gradient launch's tail (a fuse_update plan, kernels_fx.hip)
  UPD_JOINT,       // launch_update_joint: parameters and precisions
};
using TrajHook = std::function<int(int step, bool updated)>;

static TrajUpdate plan_update(const Plan& p) { return p.fuse_update ? UPD_FUSED : UPD_SEPARATE; }

// Positions first .. last of the sequence of a trajectory of L steps whose start traj_prepare
// (or the joint step's staging) has enqueued:
//   0        gradient with f(theta_0) into pred0 (the restore copy, the residual change), INIT update
//   1 .. L   gradient, update; the last gradient writes the predictions, the last update is MODE_LAST
//   L + 1    the rejected branches are back at theta_0: their prediction rows go back to f(theta_0)
// bann_hmc_step, hmc_step_tail and bann_hmc_step_joint run 0 .. L + 1 in one call, launch by
// launch or inside a stream capture; a leapfrog session walks through it call by call.
// hook (nullable): at 1 .. L, after the gradient launch (false) and after the update launch
// (true).  UPD_FUSED has no point between the two: a caller with a hook does not ask for it.
// marks: the launch-timing marks of a leapfrog session (no-ops unless bann_set_launch_timing).
// Never inside a capture, where a recorded event would become a graph node.  A step that
// follows another within the call starts where that one ended (tm_mark_follow); between two
// calls the caller may have enqueued work of its own, so a call's first step marks afresh.
static int traj_run(bann_ctx* ctx, const Plan& p, int32_t L, int32_t first, int32_t last, TrajUpdate upd,
                    const TrajHook* hook, bool marks) {
  const int32_t nb = (int32_t)p.all.size();
  for (int32_t k = first; k <= std::min(last, L); ++k) {
    const int write_pred = k == 0 ? 2 : (k == L ? 1 : 0);
    const int mode = k == 0 ? MODE_INIT : (k < L ? MODE_STEP : MODE_LAST);
    const bool hooked = hook && k >= 1;
    if (marks) (k == first ? tm_mark : tm_mark_follow)(ctx, TM_GRAD0);
    if (upd == UPD_FUSED) mark_predictions(ctx, p, false);  // theta moves in the gradient launch
    int rc = upd == UPD_FUSED ? run_grad(ctx, p, write_pred, mode, k) : run_grad(ctx, p, write_pred);
    if (marks) tm_mark(ctx, TM_GRAD1);  // UPD_FUSED: the timing books both on the gradient
    if (rc) return rc;
    if (hooked && (rc = (*hook)(k, false))) return rc;
    if (upd == UPD_SEPARATE) run_update(ctx, p, mode, k);
    if (upd == UPD_JOINT) launch_update_joint(ctx->st, p.d_all, nb, mode, k, ctx->stream);
    if (hooked && (rc = (*hook)(k, true))) return rc;
    if (marks) tm_mark(ctx, TM_UPD1);
  }
  if (last > L) launch_restore_pred(ctx->st, p.d_all, nb, ctx->stream);
  CK(hipGetLastError());
  return BANN_OK;
}

// the whole sequence of a plan shape captured once into a HIP graph and replayed
static int traj_replay(bann_ctx* ctx, const Plan& p, int32_t L) {
  const std::string key = traj_graph_key(ctx, p, L);
  hipGraphExec_t exec = nullptr;
  for (auto& e : ctx->graphs)
    if (e.first == key) exec = e.second;
  if (!exec) {
    if (ctx->graphs.size() >= 16) clear_graphs(ctx);
    CK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
    const int rc = traj_run(ctx, p, L, 0, L + 1, plan_update(p), nullptr, /*marks=*/false);
    hipGraph_t g = nullptr;
    const hipError_t ee = hipStreamEndCapture(ctx->stream, &g);
    if (rc) {
      if (g) (void)hipGraphDestroy(g);
      return rc;
    }
    CK(ee);
    const hipError_t ei = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    CK(ei);
    ctx->graphs.push_back({key, exec});
  }
  CK(hipGraphLaunch(exec, ctx->stream));
  return BANN_OK;
}

// A whole trajectory on the stream, its predictions marked current.  As one graph launch where
// replay is on and nothing has to happen between the launches; with a hook (recording) launch
// by launch with the gradient and the update apart, whatever the plan could fuse.
static int traj_whole(bann_ctx* ctx, const Plan& p, int32_t L, bool joint, const TrajHook* hook) {
  int rc;
  if (ctx->graph_replay && !joint && !hook)
    rc = traj_replay(ctx, p, L);
  else
    rc = traj_run(ctx, p, L, 0, L + 1, joint ? UPD_JOINT : (hook ? UPD_SEPARATE : plan_update(p)), hook, false);
  if (rc) return rc;
  mark_predictions(ctx, p, true);
  return BANN_OK;
}

extern "C" int bann_hmc_step(bann_ctx* ctx, const int32_t* branches, int32_t nb, int32_t L, float max_dh,
                             int32_t step_mode, float factor, const float* eps, const float* momentum, uint64_t seed,
                             const float* u, int32_t* status_out, double* h_trace_out, int32_t* uturn_out,
                             double* log_density_out) {
  if (!ctx || !ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (!branches || nb <= 0 || L < 0) return fail(ctx, BANN_E_ARG, "bad branch list or L");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  Plan p;
  int rc = build_plan(ctx, branches, nb, p, false);  // refuses a duplicate branch, before anything is touched
  if (rc) return rc;
  rc = traj_prepare(ctx, p, std::max(L, 1), max_dh, step_mode, factor, eps, momentum, seed, u);
  if (rc) return rc;
  if (L == 0) {  // empty leapfrog loop: accept_or_reject at the initial state accepts
    rc = run_grad(ctx, p, 1);
    if (rc) return rc;
    run_update(ctx, p, MODE_GRAD, 0);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < nb; ++i) {
      if (status_out) status_out[i] = BANN_ACCEPTED;
      if (uturn_out) uturn_out[i] = -1;
    }
    return hmc_outputs(ctx, branches, nb, 0, nullptr, nullptr, nullptr, log_density_out);
  }
  TrajHook hook;
  if (ctx->rec_on) {
    rec_begin(ctx, branches, nb, L, false);
    hook = [=](int k, bool updated) { return rec_step(ctx, branches, nb, k, updated); };
  }
  rc = traj_whole(ctx, p, L, false, ctx->rec_on ? &hook : nullptr);
  if (rc) return rc;
  CK(hipStreamSynchronize(ctx->stream));
  if (ctx->rec_on && (rc = rec_finish(ctx, branches, nb, L))) return rc;
  return hmc_outputs(ctx, branches, nb, L, status_out, h_trace_out, uturn_out, log_density_out);
}

// The sequential driver's branch-update tail in ONE host wait (bann_net.cpp update_branch;
// net.rs:286-300): bann_hmc_step's trajectory for branch b, then -- stream-ordered, not
// waited for -- residual_from_target_shift's residual op (residual = target - f_b(final) +
// add) and the copies of the trajectory status and the final parameters into pinned
// stages: one stream synchronisation instead of three waits and two synchronous copies
// (profiles/r06_seq_api.txt).  The same launches in the same order as bann_hmc_step +
// bann_branch_get_params + residual_from_target_shift, hence the same bits.  stats: sum
// and sum of squares of the residual before and after the shift.  A recording context and
// L = 0 take those three calls as they are.
int hmc_step_tail(bann_ctx* ctx, int32_t b, int32_t L, float max_dh, int32_t step_mode, float factor, const float* eps,
                  const float* momentum, uint64_t seed, const float* u, float add, int32_t* status_out,
                  float* params_out, double* stats) {
  if (!ctx || !ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (!status_out || !params_out || !stats) return fail(ctx, BANN_E_ARG, "null output");
  if (L < 1 || ctx->rec_on) {
    int rc = bann_hmc_step(ctx, &b, 1, L, max_dh, step_mode, factor, eps, momentum, seed, u, status_out, nullptr,
                           nullptr, nullptr);
    if (rc) return rc;
    rc = bann_branch_get_params(ctx, b, params_out);
    if (rc) return rc;
    return residual_from_target_shift(ctx, b, add, &stats[0], &stats[1], &stats[2], &stats[3]);
  }
  if (!check_branch(ctx, b)) return fail(ctx, BANN_E_ARG, "bad branch");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  Plan p;
  int rc = build_plan(ctx, &b, 1, p, false);
  if (rc) return rc;
  rc = traj_prepare(ctx, p, L, max_dh, step_mode, factor, eps, momentum, seed, u);
  if (rc) return rc;
  rc = traj_whole(ctx, p, L, false, nullptr);
  if (rc) return rc;
  rc = residual_from_target_shift_launch(ctx, b, add);
  if (rc) return rc;
  const BranchHost& h = ctx->br[b];
  CK(hipMemcpyAsync(ctx->h_status + b, ctx->d_status + b, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(ctx->h_par_stage, ctx->d_theta + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost,
                    ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  *status_out = ctx->h_status[b];
  std::memcpy(params_out, ctx->h_par_stage, h.P * sizeof(float));
  for (int k = 0; k < 4; ++k) stats[k] = ctx->h_res_stat[k];
  return BANN_OK;
}

// hmc_step_joint (branch_sampler.rs:1070-1178): parameters AND precisions.  Its host staging
// is its own; the launch sequence, the trace and the read-back are bann_hmc_step's.
extern "C" int bann_hmc_step_joint(bann_ctx* ctx, const int32_t* branches, int32_t nb, int32_t L, float max_dh,
                                   int32_t step_mode, float factor, const float* eps, const float* momentum,
                                   uint64_t seed, const float* u, const float* hyper, int32_t* status_out,
                                   double* h_trace_out, double* log_density_out) {
  if (!ctx || !ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (!branches || nb <= 0 || L < 1 || !hyper) return fail(ctx, BANN_E_ARG, "bad branch list, L or hyperparameters");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  if (step_mode == BANN_STEP_INJECTED && !eps) return fail(ctx, BANN_E_ARG, "injected step sizes need eps");
  Plan p;
  int rc = build_plan(ctx, branches, nb, p, false);
  if (rc) return rc;
  int32_t max_q = 0;
  for (int i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    if (h.prior == BANN_STD_NORMAL)
      return fail(ctx, BANN_E_ARG, "std_normal has no joint density (std_normal_branch.rs:119-131)");
    if (h.dev.nq > BANN_JOINT_MAXQ) return fail(ctx, BANN_E_SHAPE, "too many precisions for the joint update");
    max_q = std::max(max_q, h.dev.nq);
  }
  rc = trace_setup(ctx, L, max_dh);
  if (rc) return rc;
  for (int k = 0; k < 6; ++k) ctx->st.hyper[k] = hyper[k];
  // host staging: precision coordinates, output-weight stats, step sizes, momenta, uniforms
  std::vector<float> ows(2 * ctx->br.size(), 0.f), ep, mo, uu(ctx->br.size(), 0.f);
  std::mt19937_64 rng(seed ^ 0x5DEECE66Dull);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  int64_t off = 0;
  for (int i = 0; i < nb; ++i) {
    const int b = branches[i];
    const BranchHost& h = ctx->br[b];
    const int P = h.P, Q = h.dev.nq;
    CK(hipMemcpyAsync(ctx->d_phi + h.dev.q_off, h.prec.data(), Q * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ows[2 * b] = h.ows_reg_sum;
    ows[2 * b + 1] = h.ows_num >= 0.f ? h.ows_num : (float)h.widths[h.L - 2];
    if (step_mode == BANN_STEP_INJECTED) {
      ep.assign(eps + off, eps + off + P + Q);
    } else {  // random_step_sizes (654-704): U(0,1) (P + Q)^-1/4 c -- the joint sampler's only mode (1092-1101)
      ep.resize(P + Q);
      const float f = powf((float)(P + Q), -0.25f) * factor;
      for (auto& e : ep) e = U(rng) * f;
    }
    CK(hipMemcpyAsync(ctx->d_eps + h.dev.p_off, ep.data(), P * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(ctx->d_ephi + h.dev.q_off, ep.data() + P, Q * sizeof(float), hipMemcpyHostToDevice,
                      ctx->stream));
    if (momentum) {
      CK(hipMemcpyAsync(ctx->d_mom + h.dev.p_off, momentum + off, P * sizeof(float), hipMemcpyHostToDevice,
                        ctx->stream));
      CK(hipMemcpyAsync(ctx->d_mphi + h.dev.q_off, momentum + off + P, Q * sizeof(float), hipMemcpyHostToDevice,
                        ctx->stream));
    }
    uu[b] = u ? u[i] : U(rng);
    off += P + Q;
    CK(hipStreamSynchronize(ctx->stream));  // ep is reused
  }
  CK(hipMemcpyAsync(ctx->d_ows, ows.data(), ows.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(ctx->d_u, uu.data(), uu.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (!momentum) {
    launch_sample_momentum(ctx->st, p.d_all, nb, p.max_p, seed, ctx->stream);
    launch_sample_momentum_joint(ctx->st, p.d_all, nb, max_q, seed, ctx->stream);
  }
  CK(trace_clear(ctx));
  mark_predictions(ctx, p, false);  // theta moves (launch_update_joint does not go through run_update)
  TrajHook hook;
  if (ctx->rec_on) {
    rec_begin(ctx, branches, nb, L, true);
    hook = [=](int k, bool updated) { return rec_step(ctx, branches, nb, k, updated); };
  }
  rc = traj_whole(ctx, p, L, true, ctx->rec_on ? &hook : nullptr);
  if (rc) return rc;
  CK(hipStreamSynchronize(ctx->stream));
  if (ctx->rec_on && (rc = rec_finish(ctx, branches, nb, L))) return rc;
  rc = hmc_outputs(ctx, branches, nb, L, status_out, h_trace_out, nullptr, log_density_out);
  if (rc) return rc;
  for (int i = 0; i < nb; ++i) {  // the sampled precisions become the branch's (host copy and derived device arrays)
    BranchHost& h = ctx->br[branches[i]];
    CK(hipMemcpy(h.prec.data(), ctx->d_phi + h.dev.q_off, h.dev.nq * sizeof(float), hipMemcpyDeviceToHost));
    rc = upload_precisions(ctx, branches[i]);
    if (rc) return rc;
  }
  return BANN_OK;
}

extern "C" int bann_set_trajectory_recording(bann_ctx* ctx, int32_t enabled) {
  if (!ctx) return BANN_E_ARG;
  ctx->rec_on = enabled != 0;
  return BANN_OK;
}

extern "C" int bann_branch_get_trajectory(bann_ctx* ctx, int32_t b, int32_t cap, int32_t* steps, float* params,
                                          float* ldg, double* hamiltonian) {
  if (!check_branch(ctx, b)) return fail(ctx, BANN_E_ARG, "bad branch");
  if (b >= (int32_t)ctx->rec.size() || ctx->rec[b].h.empty()) return fail(ctx, BANN_E_STATE, "no recorded trajectory");
  const auto& R = ctx->rec[b];
  if (R.q) return fail(ctx, BANN_E_STATE, "the last recorded trajectory is joint (bann_branch_get_trajectory_joint)");
  const int64_t P = ctx->br[b].P;
  const int32_t k = std::min(cap, R.steps);
  if (steps) *steps = R.steps;
  if (params) std::copy(R.params.begin(), R.params.begin() + k * P, params);
  if (ldg) std::copy(R.ldg.begin(), R.ldg.begin() + k * P, ldg);
  if (hamiltonian) std::copy(R.h.begin(), R.h.begin() + k + 1, hamiltonian);
  return BANN_OK;
}

extern "C" int bann_branch_get_trajectory_joint(bann_ctx* ctx, int32_t b, int32_t cap, int32_t* steps, float* params,
                                                float* precisions, float* ldg, double* hamiltonian) {
  if (!check_branch(ctx, b)) return fail(ctx, BANN_E_ARG, "bad branch");
  if (b >= (int32_t)ctx->rec.size() || ctx->rec[b].h.empty()) return fail(ctx, BANN_E_STATE, "no recorded trajectory");
  const auto& R = ctx->rec[b];
  if (!R.q) return fail(ctx, BANN_E_STATE, "the last recorded trajectory is not joint (bann_branch_get_trajectory)");
  const int64_t P = ctx->br[b].P, Q = R.q;
  const int32_t k = std::min(cap, R.steps);
  if (steps) *steps = R.steps;
  if (params) std::copy(R.params.begin(), R.params.begin() + k * P, params);
  if (precisions) std::copy(R.prec.begin(), R.prec.begin() + k * Q, precisions);
  if (ldg) std::copy(R.ldg.begin(), R.ldg.begin() + k * (P + Q), ldg);
  if (hamiltonian) std::copy(R.h.begin(), R.h.begin() + k + 1, hamiltonian);
  return BANN_OK;
}

// ---- in-trajectory launch timing (bann_set_launch_timing) ----
// an event at every launch boundary: TM_GRAD0 before a gradient launch, TM_GRAD1
// between the gradient and the update launch, TM_UPD1 after the update; network
// mode adds TM_FWD0/1 around the forward launch and TM_AR0/1 around the all-reduce
void tm_mark(bann_ctx* ctx, int32_t kind) {
  if (!ctx->tm_on) return;
  // the next unused event of the pool (a follow mark reuses its predecessor's event)
  const size_t k = ctx->tm_marks.empty() ? 0 : (size_t)ctx->tm_marks.back().first + 1;
  if (k == ctx->tm_pool.size()) {
    hipEvent_t e;
    // timing only (resolved after a stream synchronisation): no system-scope fence on
    // record -- with it every mark wrote back and invalidated the caches between two
    // launches (the N = 8 shard's line: 4 477 vs 4 656 steps/s with marks vs without)
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;  // best effort: no sample
    ctx->tm_pool.push_back(e);
  }
  if (hipEventRecord(ctx->tm_pool[k], ctx->stream) != hipSuccess) return;
  ctx->tm_marks.push_back({(int32_t)k, kind});
}

// after the stream has drained: elapsed time of every (start, end) pair of marks
// a mark that starts where the previous mark (an update's end) left off, with nothing
// enqueued in between: the same event, no second record on the stream
void tm_mark_follow(bann_ctx* ctx, int32_t kind) {
  if (!ctx->tm_on) return;
  if (!ctx->tm_marks.empty() && ctx->tm_marks.back().second == TM_UPD1) {
    ctx->tm_marks.push_back({ctx->tm_marks.back().first, kind});
    return;
  }
  tm_mark(ctx, kind);
}

int tm_resolve(bann_ctx* ctx) {
  for (size_t i = 0; i + 1 < ctx->tm_marks.size(); ++i) {
    const auto a = ctx->tm_marks[i], b = ctx->tm_marks[i + 1];
    double* acc = nullptr;
    int32_t* cnt = nullptr;
    if (a.second == TM_GRAD0 && b.second == TM_GRAD1) acc = &ctx->tm_grad_ms, cnt = &ctx->tm_grad_n;
    else if (a.second == TM_GRAD1 && b.second == TM_UPD1) acc = &ctx->tm_upd_ms, cnt = &ctx->tm_upd_n;
    else if (a.second == TM_FWD0 && b.second == TM_FWD1) acc = &ctx->tm_fwd_ms, cnt = &ctx->tm_fwd_n;
    else if (a.second == TM_AR0 && b.second == TM_AR1) acc = &ctx->tm_ar_ms, cnt = &ctx->tm_ar_n;
    if (!acc) continue;
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, ctx->tm_pool[a.first], ctx->tm_pool[b.first]));
    *acc += ms;
    ++*cnt;
  }
  ctx->tm_marks.clear();
  return BANN_OK;
}

extern "C" int bann_set_launch_timing(bann_ctx* ctx, int32_t enabled) {
  if (!ctx) return BANN_E_ARG;
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  ctx->tm_on = enabled != 0;
  ctx->tm_marks.clear();
  return BANN_OK;
}

extern "C" int bann_launch_timing(bann_ctx* ctx, float* grad_ms, float* update_ms, int32_t* grad_launches,
                                  int32_t reset) {
  if (!ctx) return BANN_E_ARG;
  if (grad_ms) *grad_ms = ctx->tm_grad_n ? (float)(ctx->tm_grad_ms / ctx->tm_grad_n) : 0.f;
  if (update_ms) *update_ms = ctx->tm_upd_n ? (float)(ctx->tm_upd_ms / ctx->tm_upd_n) : 0.f;
  if (grad_launches) *grad_launches = ctx->tm_grad_n;
  if (reset) {
    ctx->tm_grad_ms = ctx->tm_upd_ms = 0.0;
    ctx->tm_grad_n = ctx->tm_upd_n = 0;
  }
  return BANN_OK;
}

extern "C" int bann_network_timing(bann_ctx* ctx, float* forward_ms, float* allreduce_ms, int32_t* allreduces,
                                   int32_t reset) {
  if (!ctx) return BANN_E_ARG;
  if (forward_ms) *forward_ms = ctx->tm_fwd_n ? (float)(ctx->tm_fwd_ms / ctx->tm_fwd_n) : 0.f;
  if (allreduce_ms) *allreduce_ms = ctx->tm_ar_n ? (float)(ctx->tm_ar_ms / ctx->tm_ar_n) : 0.f;
  if (allreduces) *allreduces = ctx->tm_ar_n;
  if (reset) {
    ctx->tm_fwd_ms = ctx->tm_ar_ms = 0.0;
    ctx->tm_fwd_n = ctx->tm_ar_n = 0;
  }
  return BANN_OK;
}

// ---- the leapfrog session: traj_run's sequence call by call, with the launch-timing marks ----
extern "C" int bann_leapfrog_begin(bann_ctx* ctx, const int32_t* branches, int32_t nb, int32_t L, float max_dh,
                                   int32_t step_mode, float factor, uint64_t seed) {
  if (!ctx || !ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is already active (call bann_leapfrog_end)");
  if (!branches || nb <= 0 || L < 1) return fail(ctx, BANN_E_ARG, "bad branch list or L");
  int rc = BANN_OK;
  // the packed launch plan of a branch set is reused across trajectories (a sweep
  // runs the same set every time); rebuild only when the set changes
  if (!(ctx->lf.owns && ctx->lf.all.size() == (size_t)nb && std::equal(branches, branches + nb, ctx->lf.all.begin()))) {
    rc = build_plan(ctx, branches, nb, ctx->lf, true);
    if (rc) return rc;
  }
  rc = traj_prepare(ctx, ctx->lf, L, max_dh, step_mode, factor, nullptr, nullptr, seed, nullptr);
  if (rc) return rc;
  rc = traj_run(ctx, ctx->lf, L, 0, 0, plan_update(ctx->lf), nullptr, /*marks=*/true);
  if (rc) return rc;
  ctx->lf_active = true;
  ctx->lf_L = L;
  ctx->lf_step = 0;
  return BANN_OK;
}

extern "C" int bann_leapfrog_steps(bann_ctx* ctx, int32_t k) {
  if (!ctx || !ctx->lf_active) return fail(ctx, BANN_E_STATE, "no leapfrog session");
  if (k < 0 || ctx->lf_step + k > ctx->lf_L) return fail(ctx, BANN_E_ARG, "steps beyond the trajectory length");
  const int32_t first = ctx->lf_step + 1;
  ctx->lf_step += k;
  return traj_run(ctx, ctx->lf, ctx->lf_L, first, ctx->lf_step, plan_update(ctx->lf), nullptr, /*marks=*/true);
}

extern "C" int bann_leapfrog_end(bann_ctx* ctx, int32_t* status_out, int32_t* num_accepted) {
  if (!ctx || !ctx->lf_active) return fail(ctx, BANN_E_STATE, "no leapfrog session");
  if (ctx->lf_step != ctx->lf_L) {
    int rc = bann_leapfrog_steps(ctx, ctx->lf_L - ctx->lf_step);
    if (rc) return rc;
  }
  int rc = traj_run(ctx, ctx->lf, ctx->lf_L, ctx->lf_L + 1, ctx->lf_L + 1, plan_update(ctx->lf), nullptr, false);
  if (rc) return rc;
  mark_predictions(ctx, ctx->lf, true);
  CK(hipMemcpyAsync(ctx->h_status, ctx->d_status, ctx->br.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                    ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  rc = tm_resolve(ctx);
  if (rc) return rc;
  const int32_t* st = ctx->h_status;
  int acc = 0;
  for (size_t i = 0; i < ctx->lf.all.size(); ++i) {
    const int s = st[ctx->lf.all[i]];
    if (status_out) status_out[i] = s;
    acc += s == BANN_ACCEPTED;
  }
  if (num_accepted) *num_accepted = acc;
  ctx->lf_active = false;
  return BANN_OK;
}

extern "C" int bann_leapfrog_residual_delta_device(bann_ctx* ctx, float* out_device) {
  if (!ctx || !out_device) return BANN_E_ARG;
  if (ctx->lf.all.empty() || ctx->lf_active) return fail(ctx, BANN_E_STATE, "call after bann_leapfrog_end");
  launch_residual_delta(ctx->st, ctx->lf.d_all, (int32_t)ctx->lf.all.size(), ctx->d_delta_part, out_device,
                        ctx->stream);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_leapfrog_residual_delta(bann_ctx* ctx, float* out_host) {
  if (!ctx || !out_host) return BANN_E_ARG;
  if (ctx->lf.all.empty() || ctx->lf_active) return fail(ctx, BANN_E_STATE, "call after bann_leapfrog_end");
  launch_residual_delta(ctx->st, ctx->lf.d_all, (int32_t)ctx->lf.all.size(), ctx->d_delta_part, ctx->d_delta,
                        ctx->stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->h_delta, ctx->d_delta, ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  memcpy(out_host, ctx->h_delta, ctx->n * sizeof(float));
  return BANN_OK;
}

extern "C" int bann_leapfrog_predictions_device(bann_ctx* ctx, float** out) {
  if (!ctx || !out) return BANN_E_ARG;
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "predictions are current after bann_leapfrog_end");
  *out = ctx->d_pred;
  return BANN_OK;
}

extern "C" int bann_profile_session(bann_ctx* ctx, int32_t iters, float* grad_ms, float* update_ms) {
  if (!ctx || !ctx->lf_active) return fail(ctx, BANN_E_STATE, "no leapfrog session");
  if (iters <= 0) return fail(ctx, BANN_E_ARG, "iters must be positive");
  hipEvent_t e0, e1, e2;
  CK(hipEventCreateWithFlags(&e0, hipEventDisableSystemFence));  // timing only
  CK(hipEventCreateWithFlags(&e1, hipEventDisableSystemFence));
  CK(hipEventCreateWithFlags(&e2, hipEventDisableSystemFence));
  CK(hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < iters; ++i) {
    int rc = run_grad(ctx, ctx->lf, 0);
    if (rc) return rc;
  }
  CK(hipEventRecord(e1, ctx->stream));
  for (int i = 0; i < iters; ++i) run_update(ctx, ctx->lf, MODE_PROFILE, 1);
  CK(hipEventRecord(e2, ctx->stream));
  CK(hipEventSynchronize(e2));
  float t01 = 0.f, t12 = 0.f;
  CK(hipEventElapsedTime(&t01, e0, e1));
  CK(hipEventElapsedTime(&t12, e1, e2));
  if (grad_ms) *grad_ms = t01 / iters;
  if (update_ms) *update_ms = t12 / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipEventDestroy(e2);
  return BANN_OK;
}
