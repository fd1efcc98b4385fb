// skyjo_learner.hip - the packed nets' handles and the learner behind the extern "C" boundary of include/skyjo_vec.h: skyjo_vec_mlp_*,
// skyjo_vec_rollout_targets / _select / _gather / _gather_logits / _shuffle, skyjo_vec_ppo_loss / _kl, skyjo_vec_mlp_train_*, skyjo_vec_grad_norm, skyjo_vec_ppo_update,
// skyjo_vec_arena_* and skyjo_vec_episode_stats,
// with their kernels (skyjo_update.h, skyjo_clip.h, skyjo_targets.h, skyjo_batches.h, skyjo_loss.h, skyjo_train.h, skyjo_train_wide.h, skyjo_epoch.h, skyjo_arena.h; what they share: skyjo_learner_util.h).  A translation unit and a code object of its own: nothing here is part of the environment's sources
// (skyjo_capi.hip, skyjo_device.h and its parts), and of an engine it sees what skyjo_host.h shows - the record layout, B, G, game_id0,
// the device and the select scratch.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "skyjo_host.h"
#include "skyjo_learner_util.h"
#include "skyjo_update.h"
#include "skyjo_clip.h"
#include "skyjo_targets.h"
#include "skyjo_batches.h"
#include "skyjo_loss.h"
#include "skyjo_train.h"
#include "skyjo_train_wide.h"
#include "skyjo_epoch.h"
#include "skyjo_arena.h"

extern "C" {

int skyjo_vec_mlp_create(int32_t device_id, int32_t obs_dim, int32_t out_dim, int32_t precision, const float *w1, const float *b1,
                         const float *w2, const float *b2, const float *w3, const float *b3, skyjo_vec_mlp **out) {
  if (!out || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return fail(SKYJO_E_INVALID, "null argument");
  if (obs_dim < 1 || obs_dim > SKP_MAX_OBS || out_dim < 1 || out_dim > SKP_OUT)
    return fail(SKYJO_E_INVALID, "skyjo_vec_mlp: obs_dim must be 1..163 and out_dim 1..32");
  if (precision != SKYJO_MLP_BF16 && precision != SKYJO_MLP_FP32) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp: unknown precision");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return fail(SKYJO_E_INVALID, "device_id out of range");
  DevGuard guard_(device_id);
  const bool split = precision == SKYJO_MLP_FP32;
  skyjo_vec_mlp *m = new skyjo_vec_mlp();
  m->device_id = device_id, m->obs_dim = obs_dim, m->out_dim = m->net.out_dim = out_dim;
  if (hipMalloc(&m->blob, skp_piece_offset(8, split, skp_w1_ksteps(obs_dim))) != hipSuccess) {
    delete m;
    return fail(SKYJO_E_DEVICE, "hipMalloc failed for the packed weights");
  }
  // k_mlp_update packs (skyjo_update.h).  The host arrays are staged the way the Adam state lies: tensor i at sku_tensor_offset(i).  Every
  // tensor in front of w2 and of w3 is a multiple of SKP_HIDDEN floats, so the two are 16-byte aligned as sku_elem4 needs them.
  static_assert(SKP_HIDDEN % 4 == 0, "w2 and w3 are staged at multiples of SKP_HIDDEN floats: sku_elem4 reads them 16 bytes at a time");
  SkUpdArgs a{};
  skp_blob_views(m->blob, split, obs_dim, m->net, a);
  a.obs_dim = obs_dim, a.out_dim = out_dim;
  const float *const src[SKU_TENSORS] = {w1, b1, w2, b2, w3, b3};
  DevBuf stage;
  const char *what = "hipMalloc";
  hipError_t e = hipMalloc(&stage.p, sku_state_half(obs_dim, out_dim) * sizeof(float));
  for (int i = 0; i < SKU_TENSORS && e == hipSuccess; i++) {
    a.p[i] = (float *)stage.p + sku_tensor_offset(i, obs_dim, out_dim);
    what = "hipMemcpy", e = hipMemcpy(a.p[i], src[i], sku_tensor_elems(i, obs_dim, out_dim) * sizeof(float), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_mlp_update<false>, dim3(SKU_BLOCKS), dim3(SKU_THREADS), 0, nullptr, a);
    what = "k_mlp_update", e = hipGetLastError();
  }
  if (e == hipSuccess) what = "hipStreamSynchronize", e = hipStreamSynchronize(nullptr);  // (the staging area is freed on return)
  if (e != hipSuccess) {
    (void)hipFree(m->blob);
    delete m;
    return fail(SKYJO_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
  }
  *out = m;
  return SKYJO_OK;
}

int skyjo_vec_mlp_destroy(skyjo_vec_mlp *m) {
  if (!m) return SKYJO_OK;
  DevGuard guard_(m->device_id);
  (void)hipFree(m->blob);
  delete m;
  return SKYJO_OK;
}

// ---- the packed net rewritten in place from device memory (include/skyjo_vec.h: skyjo_vec_mlp_update / _adam_step; skyjo_update.h) ----
namespace {

// k_mlp_update's view of the blob and the net's dimensions, with a call's tensors
bool mlp_update_args(const skyjo_vec_mlp *m, const float *const p[SKU_TENSORS], SkUpdArgs &a) {
  SkMlpDev net{};  // (the net kernels' view of the same blob: m->net holds it already)
  skp_blob_views(m->blob, m->net.split != 0, m->obs_dim, net, a);
  a.obs_dim = m->obs_dim, a.out_dim = m->out_dim;
  for (int i = 0; i < SKU_TENSORS; i++) {
    if (!p[i]) return false;
    a.p[i] = const_cast<float *>(p[i]);
  }
  return true;
}
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int skyjo_vec_mlp_update(skyjo_vec_mlp *m, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                         const float *b3, void *stream) {
  const float *const p[SKU_TENSORS] = {w1, b1, w2, b2, w3, b3};
  SkUpdArgs a{};
  if (!m || !mlp_update_args(m, p, a)) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_update: null argument");
  if (!aligned16(w2) || !aligned16(w3)) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_update: w2 and w3 must be 16-byte aligned");
  DevGuard guard_(m->device_id);
  hipLaunchKernelGGL(k_mlp_update<false>, dim3(SKU_BLOCKS), dim3(SKU_THREADS), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int64_t skyjo_vec_mlp_adam_state_bytes(const skyjo_vec_mlp *m) {
  return m ? (int64_t)(2 * sku_state_half(m->obs_dim, m->out_dim) * sizeof(float)) : 0;
}

// torch.optim.Adam's scalars of a step, in double from the float32 hyper-parameters and the step, rounded to float32 once
static void adam_scalars(SkUpdArgs &a, float lr, float beta1, float beta2, float eps, int64_t step) {
  const double b1 = (double)beta1, b2 = (double)beta2, t = (double)step;
  a.w1 = (float)(1.0 - b1), a.beta2 = beta2, a.w2 = (float)(1.0 - b2);
  a.step_size = (float)((double)lr / (1.0 - std::pow(b1, t)));
  a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, t));
  a.eps = eps;
}

// both Adam entries and skyjo_vec_ppo_update: the checks and the kernel's arguments, nothing launched.  coef: the clipped entry's
// coefficient on the device, or null
static int adam_check(const char *who, skyjo_vec_mlp *m, float *const params[6], const float *const grads[6], void *state, int64_t state_bytes,
                      float lr, float beta1, float beta2, float eps, int64_t step, const float *coef, SkUpdArgs &a) {
  const std::string name(who);
  if (!m || !params || !grads || !state || !mlp_update_args(m, params, a)) return fail(SKYJO_E_INVALID, name + ": null argument");
  for (int i = 0; i < SKU_TENSORS; i++) {
    if (!grads[i]) return fail(SKYJO_E_INVALID, name + ": null gradient");
    a.g[i] = grads[i];
    a.off[i] = sku_tensor_offset(i, m->obs_dim, m->out_dim);
  }
  if (state_bytes < skyjo_vec_mlp_adam_state_bytes(m))
    return fail(SKYJO_E_INVALID, name + ": state_bytes is less than skyjo_vec_mlp_adam_state_bytes");
  if (step < 1) return fail(SKYJO_E_INVALID, name + ": step counts from 1");
  if (!std::isfinite(lr)) return fail(SKYJO_E_INVALID, name + ": lr must be finite");
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(SKYJO_E_INVALID, name + ": beta1 and beta2 must lie in [0, 1)");
  if (!(std::isfinite(eps) && eps >= 0.f)) return fail(SKYJO_E_INVALID, name + ": eps must be finite and not negative");
  if (!aligned16(state) || !aligned16(params[2]) || !aligned16(params[4]) || !aligned16(grads[2]) || !aligned16(grads[4]))
    return fail(SKYJO_E_INVALID, name + ": state, w2, w3 and their gradients must be 16-byte aligned");
  a.coef = coef;
  a.m = (float *)state, a.v = a.m + sku_state_half(m->obs_dim, m->out_dim);
  adam_scalars(a, lr, beta1, beta2, eps, step);
  return SKYJO_OK;
}
static int adam_launch(const skyjo_vec_mlp *m, const SkUpdArgs &a, hipStream_t s) {
  DevGuard guard_(m->device_id);
  hipLaunchKernelGGL(k_mlp_update<true>, dim3(SKU_BLOCKS), dim3(SKU_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}
static int adam_step(const char *who, skyjo_vec_mlp *m, float *const params[6], const float *const grads[6], void *state, int64_t state_bytes,
                     float lr, float beta1, float beta2, float eps, int64_t step, const float *coef, void *stream) {
  SkUpdArgs a{};
  if (int rc = adam_check(who, m, params, grads, state, state_bytes, lr, beta1, beta2, eps, step, coef, a)) return rc;
  return adam_launch(m, a, (hipStream_t)stream);
}

int skyjo_vec_mlp_adam_step(skyjo_vec_mlp *m, float *const params[6], const float *const grads[6], void *state, int64_t state_bytes,
                            float lr, float beta1, float beta2, float eps, int64_t step, void *stream) {
  return adam_step("skyjo_vec_mlp_adam_step", m, params, grads, state, state_bytes, lr, beta1, beta2, eps, step, nullptr, stream);
}

int skyjo_vec_mlp_adam_step_clipped(skyjo_vec_mlp *m, float *const params[6], const float *const grads[6], void *state, int64_t state_bytes,
                                    float lr, float beta1, float beta2, float eps, int64_t step, const float *coef_device, void *stream) {
  static const char *who = "skyjo_vec_mlp_adam_step_clipped";
  if (!coef_device) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if ((uintptr_t)coef_device & 3) return fail(SKYJO_E_INVALID, std::string(who) + ": coef_device is not aligned to its element size");
  return adam_step(who, m, params, grads, state, state_bytes, lr, beta1, beta2, eps, step, coef_device, stream);
}

// ---- the global L2 norm of a list of tensors and torch's clipping coefficient (include/skyjo_vec.h: skyjo_vec_grad_norm; skyjo_clip.h) ----
// the checks and the kernel's arguments, nothing launched
static int grad_norm_check(const char *who, const float *const tensors[], const int64_t counts[], int32_t n, float max_norm, float *out2, SkNormArgs &a) {
  if (!tensors || !counts || !out2) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if (n < 1 || n > SKC_MAX_SEGMENTS) return fail(SKYJO_E_INVALID, std::string(who) + ": n must lie in 1 .. 32");
  if (!(max_norm > 0.f)) return fail(SKYJO_E_INVALID, std::string(who) + ": max_norm must be greater than 0 (+inf: measure only)");
  if ((uintptr_t)out2 & 3) return fail(SKYJO_E_INVALID, std::string(who) + ": out2 is not aligned to its element size");
  for (int i = 0; i < n; i++) {
    if (counts[i] < 0) return fail(SKYJO_E_INVALID, std::string(who) + ": a count is negative");
    if (!tensors[i] && counts[i] > 0) return fail(SKYJO_E_INVALID, std::string(who) + ": a null tensor with a count greater than 0");
    if ((uintptr_t)tensors[i] & 3) return fail(SKYJO_E_INVALID, std::string(who) + ": a tensor is not aligned to its element size");
    a.ptr[i] = tensors[i], a.count[i] = (long long)counts[i];
  }
  a.n = n, a.max_norm = max_norm, a.out = out2;
  return SKYJO_OK;
}
static int grad_norm_launch(const SkNormArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_grad_norm, dim3(1), dim3(SKC_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}
int skyjo_vec_grad_norm(const float *const tensors[], const int64_t counts[], int32_t n, float max_norm, float *out2, void *stream) {
  SkNormArgs a{};
  if (int rc = grad_norm_check("skyjo_vec_grad_norm", tensors, counts, n, max_norm, out2, a)) return rc;
  return grad_norm_launch(a, (hipStream_t)stream);
}

int64_t skyjo_vec_mlp_packed_bytes(const skyjo_vec_mlp *m) {
  if (!m) return 0;
  size_t n = 0;
  for (int k = 0; k < 8; k++) n += skp_piece_bytes(k, m->net.split != 0, skp_w1_ksteps(m->obs_dim));
  return (int64_t)n;
}

int skyjo_vec_mlp_export(const skyjo_vec_mlp *m, void *dst_device, int64_t bytes, void *stream) {
  if (!m || !dst_device) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_export: null argument");
  if (bytes < skyjo_vec_mlp_packed_bytes(m)) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_export: bytes is less than skyjo_vec_mlp_packed_bytes");
  DevGuard guard_(m->device_id);
  size_t at = 0;
  for (int k = 0; k < 8; k++) {
    const size_t n = skp_piece_bytes(k, m->net.split != 0, skp_w1_ksteps(m->obs_dim));
    if (!n) continue;
    HIPCHK(hipMemcpyAsync((uint8_t *)dst_device + at, (const uint8_t *)m->blob + skp_piece_offset(k, m->net.split != 0, skp_w1_ksteps(m->obs_dim)), n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    at += n;
  }
  return SKYJO_OK;
}

int skyjo_vec_mlp_forward_layout(const skyjo_vec_mlp *m, const void *records, int32_t record_bytes, int32_t layout, int64_t n, float *out,
                                 void *stream) {
  if (!m || !records || !out || n < 0 || record_bytes < 32 || (record_bytes & 15))
    return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_forward: bad argument");
  if (int rc = check_layout(layout)) return rc;
  if (record_bytes < 16 * skp_w1_ksteps(m->obs_dim))
    return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_forward: record_bytes must hold layer 1's 16 * (obs_dim / 16 + 1) columns");
  if (n == 0) return SKYJO_OK;
  DevGuard guard_(m->device_id);
  SkMlpDraw nodraw{};
  return launch_mlp(m, m, 1, (const uint8_t *)records, (int)record_bytes, m->obs_dim, n, out, nodraw, nullptr, (hipStream_t)stream,
                    (int)(layout == SKYJO_REC_TILE_PLANAR));
}
int skyjo_vec_mlp_forward(const skyjo_vec_mlp *m, const void *records, int32_t record_bytes, int64_t n, float *out,
                          void *stream) {
  return skyjo_vec_mlp_forward_layout(m, records, record_bytes, SKYJO_REC_ROW_MAJOR, n, out, stream);
}

int skyjo_vec_mlp_act_value_layout(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, const void *records, int32_t layout,
                                   int64_t n, uint64_t seed, uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                                   float *logits_out, float *values_out, void *stream) {
  if (!h || !policy || !records || !actions_out || n < 0 || (value && !values_out))
    return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_act_value: bad argument");
  if (int rc = check_layout(layout)) return rc;
  const SkEngineView e = sk_engine_view(h);
  DevGuard guard_(e.device_id);
  if (policy->net.out_dim != SKYJO_NUM_ACTIONS) return fail(SKYJO_E_INVALID, "the policy net needs 26 outputs");
  if (value && (policy->obs_dim != value->obs_dim || policy->device_id != value->device_id || policy->device_id != e.device_id ||
                policy->net.split != value->net.split))
    return fail(SKYJO_E_INVALID, "policy and value net must share the observation size, the precision and the engine's device");
  if ((int)e.L->rec_bytes < 16 * skp_w1_ksteps(policy->obs_dim))
    return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_act_value: the engine's records are shorter than the net's layer 1 (obs_dim)");
  if (n == 0) return SKYJO_OK;
  SkMlpDraw d{};
  d.enable = 1, d.mask_offset = e.L->Dp, d.no_masking = no_masking, d.seed = seed, d.ticket = ticket;
  d.game_id0 = e.game_id0, d.actions = actions_out, d.logp = logp_out;
  return launch_mlp(policy, value ? value : policy, value ? 2 : 1, (const uint8_t *)records, (int)e.L->rec_bytes, policy->obs_dim, n, logits_out,
                    d, value ? values_out : nullptr, (hipStream_t)stream, (int)(layout == SKYJO_REC_TILE_PLANAR));
}
int skyjo_vec_mlp_act(skyjo_vec *h, const skyjo_vec_mlp *m, const void *records, int64_t n, uint64_t seed, uint64_t ticket,
                      int32_t no_masking, int32_t *actions_out, float *logp_out, float *logits_out, void *stream) {
  if (!m) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_act: bad argument");
  return skyjo_vec_mlp_act_value_layout(h, m, nullptr, records, SKYJO_REC_ROW_MAJOR, n, seed, ticket, no_masking, actions_out, logp_out, logits_out,
                                        nullptr, stream);
}
int skyjo_vec_mlp_act_value(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, const void *records, int64_t n,
                            uint64_t seed, uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                            float *logits_out, float *values_out, void *stream) {
  if (!value || !values_out) return fail(SKYJO_E_INVALID, "skyjo_vec_mlp_act_value: bad argument");
  return skyjo_vec_mlp_act_value_layout(h, policy, value, records, SKYJO_REC_ROW_MAJOR, n, seed, ticket, no_masking, actions_out, logp_out,
                                        logits_out, values_out, stream);
}

// ---- learner targets of a rollout buffer (include/skyjo_vec.h: skyjo_vec_rollout_targets; the kernel: skyjo_targets.h) ----
int skyjo_vec_rollout_targets(skyjo_vec *h, const void *records, int32_t layout, int32_t T, const float *values, int32_t value_stride,
                              const double *final_rewards, const uint8_t *episode_end, float gamma, float lambda, float *advantages_out,
                              float *value_targets_out, float *returns_out, uint8_t *flags_out, void *stream) {
  if (!h || !records || !values || !final_rewards || !episode_end || !advantages_out || !value_targets_out || !returns_out || !flags_out)
    return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_targets: null argument");
  if (T < 1 || value_stride < 1) return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_targets: T and value_stride must be at least 1");
  if (!(gamma >= 0.f && gamma <= 1.f) || !(lambda >= 0.f && lambda <= 1.f))
    return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_targets: gamma and lambda must lie in [0, 1]");
  if (int rc = check_layout(layout)) return rc;
  const SkEngineView e = sk_engine_view(h);
  DevGuard guard_(e.device_id);
  const SkLayout &L = *e.L;
  SkTargetsArgs a{};
  a.rec = sk_records(e, records, layout), a.values = values, a.rewards = final_rewards, a.end = episode_end;
  a.adv = advantages_out, a.vt = value_targets_out, a.ret = returns_out, a.flags = flags_out;
  a.T = T, a.N = L.N, a.vstride = value_stride;
  a.off_agent = L.Dp + 26, a.off_done = L.Dp + 28;
  a.gamma = gamma, a.gl = gamma * lambda;  // (float32 product, rounded once: part of the definition)
  const dim3 grid((e.B + SK_TGT_LANES - 1) / SK_TGT_LANES), block(SK_TGT_LANES);
  switch (L.N) {
    case 2: hipLaunchKernelGGL(k_rollout_targets<2>, grid, block, 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(k_rollout_targets<3>, grid, block, 0, (hipStream_t)stream, a); break;
    case 4: hipLaunchKernelGGL(k_rollout_targets<4>, grid, block, 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(k_rollout_targets<0>, grid, block, 0, (hipStream_t)stream, a); break;
  }
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

// ---- learner minibatches of a rollout buffer (include/skyjo_vec.h: skyjo_vec_rollout_select / _gather; the kernels: skyjo_batches.h) ----
// both entries, after their checks: the scratch, then the count pass, k_select_scan and the scatter pass.  st: the seats form's records
// and mask, or null.  n_rows == 0 launches the scan alone, which writes the zeros.
static int select_rows(skyjo_vec *h, const SkSelectSeats *st, const uint8_t *flags, int64_t n_rows, int32_t require_bits, const float *advantages,
                       int64_t *index_out, int64_t *count_out, double *moments_out, hipStream_t s) {
  const size_t nb = (size_t)((n_rows + SK_SEL_ROWS - 1) / SK_SEL_ROWS);
  void *scratch = nullptr;
  size_t cap = 0;
  if (int rc = sk_engine_select_scratch(h, nb, &scratch, &cap)) return rc;
  long long *counts = (long long *)scratch;
  double *sums = (double *)(counts + cap);
  const SkSelectSeats seats = st ? *st : SkSelectSeats{};
  const dim3 grid((unsigned)nb), block(SK_SEL_THREADS);
  const auto count = st ? k_select_pass<false, true> : k_select_pass<false, false>;
  const auto scatter = st ? k_select_pass<true, true> : k_select_pass<true, false>;
  if (nb) hipLaunchKernelGGL(count, grid, block, 0, s, flags, (long long)n_rows, (uint32_t)require_bits, advantages, counts, sums, (long long *)nullptr, seats);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(SK_SCAN_THREADS), 0, s, counts, (const double *)sums, (int)nb, (long long *)count_out, moments_out);
  HIPCHK(hipGetLastError());
  if (nb) hipLaunchKernelGGL(scatter, grid, block, 0, s, flags, (long long)n_rows, (uint32_t)require_bits, (const float *)nullptr, counts, sums, (long long *)index_out, seats);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int skyjo_vec_rollout_select(skyjo_vec *h, const uint8_t *flags, int64_t n_rows, int32_t require_bits, const float *advantages,
                             int64_t *index_out, int64_t *count_out, double *moments_out, void *stream) {
  if (!h || !flags || !index_out || !count_out) return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_select: null argument");
  if ((advantages == nullptr) != (moments_out == nullptr))
    return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_select: advantages and moments_out go together");
  if (n_rows < 0 || n_rows > (int64_t)SK_SEL_ROWS * 0x7fffffff) return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_select: n_rows out of range");
  if (require_bits < 1 || require_bits > 255) return fail(SKYJO_E_INVALID, "skyjo_vec_rollout_select: require_bits must lie in 1 .. 255");
  DevGuard guard_(sk_engine_view(h).device_id);
  return select_rows(h, nullptr, flags, n_rows, require_bits, advantages, index_out, count_out, moments_out, (hipStream_t)stream);
}

int skyjo_vec_rollout_select_seats(skyjo_vec *h, const void *records, int32_t layout, int32_t T, const uint8_t *flags, int32_t require_bits,
                                   uint32_t seat_mask, const float *advantages, int64_t *index_out, int64_t *count_out, double *moments_out,
                                   void *stream) {
  static const char *who = "skyjo_vec_rollout_select_seats";
  if (!h || !records || !flags || !index_out || !count_out) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if ((advantages == nullptr) != (moments_out == nullptr)) return fail(SKYJO_E_INVALID, std::string(who) + ": advantages and moments_out go together");
  if (T < 1) return fail(SKYJO_E_INVALID, std::string(who) + ": T must be at least 1");
  if (require_bits < 1 || require_bits > 255) return fail(SKYJO_E_INVALID, std::string(who) + ": require_bits must lie in 1 .. 255");
  if (int rc = check_layout(layout)) return rc;
  const SkEngineView e = sk_engine_view(h);
  const SkLayout &L = *e.L;
  if (seat_mask == 0u || (seat_mask >> L.N) != 0u) return fail(SKYJO_E_INVALID, std::string(who) + ": seat_mask must be non-zero and name seats below num_players only");
  const int64_t n_rows = (int64_t)T * e.B;
  if (n_rows > (int64_t)SK_SEL_ROWS * 0x7fffffff) return fail(SKYJO_E_INVALID, std::string(who) + ": T * num_envs out of range");
  DevGuard guard_(e.device_id);
  SkSelectSeats st{};
  st.rec = sk_records(e, records, layout), st.seat_mask = seat_mask, st.off_agent = L.Dp + 26;
  return select_rows(h, &st, flags, n_rows, require_bits, advantages, index_out, count_out, moments_out, (hipStream_t)stream);
}

// skyjo_vec_rollout_gather and skyjo_vec_ppo_update: the checks and the kernel's arguments, nothing launched
static int gather_check(const char *who, skyjo_vec *h, const void *records, int32_t layout, int32_t T, const int64_t *index, int64_t m,
                        const int32_t *actions, const float *logp, const float *values, int32_t value_stride, const float *advantages,
                        const float *value_targets, float adv_mean, float adv_std, float *obs_out, float *logmask_out, int64_t *actions_out,
                        float *logp_out, float *advantages_out, float *value_targets_out, float *values_out, uint8_t *seats_out, SkGatherArgs &a) {
  const std::string name(who);
  if (!h || !records || !index || !actions || !logp || !values || !advantages || !value_targets || !obs_out || !logmask_out ||
      !actions_out || !logp_out || !advantages_out || !value_targets_out || !values_out || !seats_out)
    return fail(SKYJO_E_INVALID, name + ": null argument");
  if (m < 0 || T < 1 || value_stride < 1) return fail(SKYJO_E_INVALID, name + ": m must not be negative, T and value_stride at least 1");
  if (int rc = check_layout(layout)) return rc;
  if (!std::isfinite(adv_mean) || !std::isfinite(adv_std) || !(adv_std > 0.f))
    return fail(SKYJO_E_INVALID, name + ": adv_mean must be finite, adv_std finite and greater than 0");
  if ((((uintptr_t)records | (uintptr_t)obs_out | (uintptr_t)logmask_out) & 15) != 0)
    return fail(SKYJO_E_INVALID, name + ": records, obs_out and logmask_out must be 16-byte aligned");
  const SkEngineView e = sk_engine_view(h);
  const SkLayout &L = *e.L;
  static_assert(SK_GATHER_MAX_PIECES * 16 >= ((19 + 12 * SKYJO_MAX_PLAYERS + 3) & ~3) + 32, "the largest record fits k_gather_rows' LDS image");
  a.rec = sk_records(e, records, layout), a.index = (const long long *)index, a.actions = actions, a.logp = logp, a.values = values;
  a.adv = advantages, a.vt = value_targets;
  a.obs_out = obs_out, a.lm_out = logmask_out, a.act_out = (long long *)actions_out, a.logp_out = logp_out, a.adv_out = advantages_out;
  a.vt_out = value_targets_out, a.val_out = values_out, a.seat_out = seats_out;
  a.m = m, a.n_rows = (long long)T * e.B, a.vstride = value_stride, a.D = L.D, a.Dp = L.Dp;
  a.mean = adv_mean, a.std = adv_std;
  return SKYJO_OK;
}
// a.m >= 1 rows from a.index, on the current device
static int gather_launch(const SkGatherArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((a.m + SK_GATHER_ROWS - 1) / SK_GATHER_ROWS)), dim3(SK_GATHER_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int skyjo_vec_rollout_gather(skyjo_vec *h, const void *records, int32_t layout, int32_t T, const int64_t *index, int64_t m,
                             const int32_t *actions, const float *logp, const float *values, int32_t value_stride, const float *advantages,
                             const float *value_targets, float adv_mean, float adv_std, float *obs_out, float *logmask_out,
                             int64_t *actions_out, float *logp_out, float *advantages_out, float *value_targets_out, float *values_out,
                             uint8_t *seats_out, void *stream) {
  SkGatherArgs a{};
  if (int rc = gather_check("skyjo_vec_rollout_gather", h, records, layout, T, index, m, actions, logp, values, value_stride, advantages, value_targets,
                            adv_mean, adv_std, obs_out, logmask_out, actions_out, logp_out, advantages_out, value_targets_out, values_out, seats_out, a))
    return rc;
  if (m == 0) return SKYJO_OK;
  DevGuard guard_(sk_engine_view(h).device_id);
  return gather_launch(a, (hipStream_t)stream);
}

// skyjo_vec_rollout_gather_logits and skyjo_vec_ppo_update: the checks, nothing launched
static int gather_logits_check(const char *who, const float *column, int64_t n_rows, const int64_t *index, int64_t m, float *out) {
  const std::string name(who);
  if (!column || !index || !out) return fail(SKYJO_E_INVALID, name + ": null argument");
  if (m < 0 || n_rows < 0) return fail(SKYJO_E_INVALID, name + ": m and n_rows must not be negative");
  if (!aligned16(out) || ((uintptr_t)column & 3) != 0 || ((uintptr_t)index & 7) != 0)
    return fail(SKYJO_E_INVALID, name + ": out must be 16-byte aligned, column and index aligned to their element size");
  if (m > (int64_t)SK_GATHER_ROWS * 0x7fffffff) return fail(SKYJO_E_INVALID, name + ": m is out of range");
  return SKYJO_OK;
}
static int gather_logits_launch(const float *column, int64_t n_rows, const int64_t *index, int64_t m, float *out, hipStream_t s) {
  hipLaunchKernelGGL(k_gather_logits, dim3((unsigned)((m + SK_GATHER_ROWS - 1) / SK_GATHER_ROWS)), dim3(SK_GATHER_THREADS), 0, s, column,
                     (long long)n_rows, (const long long *)index, (long long)m, out);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int skyjo_vec_rollout_gather_logits(const float *column, int64_t n_rows, const int64_t *index, int64_t m, float *out, void *stream) {
  if (int rc = gather_logits_check("skyjo_vec_rollout_gather_logits", column, n_rows, index, m, out)) return rc;
  if (m == 0) return SKYJO_OK;
  return gather_logits_launch(column, n_rows, index, m, out, (hipStream_t)stream);
}

// ---- the PPO loss head of a learner minibatch (include/skyjo_vec.h: skyjo_vec_ppo_loss, skyjo_vec_ppo_loss_kl; the kernels: skyjo_loss.h) ----
static constexpr int64_t kLossMaxRows = (int64_t)SK_LOSS_ROWS * 0x7fffffff;
static int64_t loss_scratch_bytes(int64_t m, int stats) {
  if (m < 1 || m > kLossMaxRows) return 0;
  return (m + SK_LOSS_ROWS - 1) / SK_LOSS_ROWS * (int64_t)(stats * sizeof(double));
}
int64_t skyjo_vec_ppo_loss_scratch_bytes(int64_t m) { return loss_scratch_bytes(m, SK_LOSS_STATS); }
int64_t skyjo_vec_ppo_loss_kl_scratch_bytes(int64_t m) { return loss_scratch_bytes(m, SK_LOSS_KL_STATS); }

// both entries and skyjo_vec_ppo_update: the checks and the kernel's arguments, nothing launched.  KL: old_logits and kl_coeff take
// part, seven statistics
static int ppo_loss_check(const char *who, const bool KL, const float *logits, const float *log_mask, const float *old_logits, const float *value,
                          const int64_t *actions, const float *logp_old, const float *advantages, const float *value_targets,
                          const float *values_old, int64_t m, float clip, float vf_coef, float ent_coef, float vf_clip, float kl_coeff,
                          float *grad_logits_out, float *grad_value_out, double *stats_out, void *scratch, int64_t scratch_bytes, SkLossArgs &a) {
  const std::string name(who);
  if (!logits || !log_mask || (KL && !old_logits) || !value || !actions || !logp_old || !advantages || !value_targets || !values_old ||
      !grad_logits_out || !grad_value_out || !stats_out || !scratch)
    return fail(SKYJO_E_INVALID, name + ": null argument");
  if (m < 1 || m > kLossMaxRows) return fail(SKYJO_E_INVALID, name + ": m must be at least 1");
  if (!std::isfinite(clip) || !(clip > 0.f)) return fail(SKYJO_E_INVALID, name + ": clip must be finite and greater than 0");
  if (!std::isfinite(vf_coef) || !std::isfinite(ent_coef)) return fail(SKYJO_E_INVALID, name + ": vf_coef and ent_coef must be finite");
  if (KL && (!std::isfinite(kl_coeff) || !(kl_coeff >= 0.f))) return fail(SKYJO_E_INVALID, name + ": kl_coeff must be finite and not negative");
  if ((((uintptr_t)logits | (uintptr_t)log_mask | (uintptr_t)grad_logits_out) & 15) != 0)
    return fail(SKYJO_E_INVALID, name + ": logits, log_mask and grad_logits_out must be 16-byte aligned");
  if (KL && !aligned16(old_logits)) return fail(SKYJO_E_INVALID, name + ": old_logits must be 16-byte aligned");
  if ((((uintptr_t)value | (uintptr_t)logp_old | (uintptr_t)advantages | (uintptr_t)value_targets | (uintptr_t)values_old |
        (uintptr_t)grad_value_out) & 3) != 0 || (((uintptr_t)actions | (uintptr_t)stats_out | (uintptr_t)scratch) & 7) != 0)
    return fail(SKYJO_E_INVALID, name + ": a column, stats_out or scratch is not aligned to its element size");
  const int NS = KL ? SK_LOSS_KL_STATS : SK_LOSS_STATS;
  if (scratch_bytes < loss_scratch_bytes(m, NS)) return fail(SKYJO_E_INVALID, name + ": scratch is smaller than " + name + "_scratch_bytes(m)");
  static_assert(SK_LOSS_ROWS % 2 == 0 && SK_LOSS_ROWS <= SK_LOSS_THREADS, "a run is whole 16-byte pieces and every row has its lane");
  a.logits = logits, a.log_mask = log_mask, a.old_logits = old_logits, a.value = value, a.actions = (const long long *)actions;
  a.logp_old = logp_old, a.adv = advantages, a.vt = value_targets, a.v_old = values_old, a.g_logits = grad_logits_out, a.g_value = grad_value_out;
  a.partial = (double *)scratch, a.m = m;
  a.lo = 1.0 - (double)clip, a.hi = 1.0 + (double)clip;
  a.vf_coef = vf_coef, a.ent_coef = ent_coef;
  a.vf_clip = (std::isfinite(vf_clip) && vf_clip > 0.f) ? vf_clip : 0.f;
  a.kl_coeff = kl_coeff;
  return SKYJO_OK;
}
// the main launch and the finish
static int ppo_loss_launch(const bool KL, const SkLossArgs &a, double *stats_out, hipStream_t s) {
  const int64_t m = a.m, nb = (m + SK_LOSS_ROWS - 1) / SK_LOSS_ROWS;
  const dim3 grid((unsigned)nb), one(1), threads(SK_LOSS_THREADS), fin(SK_LOSS_FIN_THREADS);
  if (KL) hipLaunchKernelGGL(k_ppo_loss<true>, grid, threads, 0, s, a);
  else hipLaunchKernelGGL(k_ppo_loss<false>, grid, threads, 0, s, a);
  HIPCHK(hipGetLastError());
  if (KL) hipLaunchKernelGGL(k_ppo_loss_finish<SK_LOSS_KL_STATS>, one, fin, 0, s, (const double *)a.partial, (int)nb, (double)m, stats_out);
  else hipLaunchKernelGGL(k_ppo_loss_finish<SK_LOSS_STATS>, one, fin, 0, s, (const double *)a.partial, (int)nb, (double)m, stats_out);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}
static int ppo_loss(const char *who, const bool KL, const float *logits, const float *log_mask, const float *old_logits, const float *value,
                    const int64_t *actions, const float *logp_old, const float *advantages, const float *value_targets,
                    const float *values_old, int64_t m, float clip, float vf_coef, float ent_coef, float vf_clip, float kl_coeff,
                    float *grad_logits_out, float *grad_value_out, double *stats_out, void *scratch, int64_t scratch_bytes, void *stream) {
  SkLossArgs a{};
  if (int rc = ppo_loss_check(who, KL, logits, log_mask, old_logits, value, actions, logp_old, advantages, value_targets, values_old, m, clip, vf_coef,
                              ent_coef, vf_clip, kl_coeff, grad_logits_out, grad_value_out, stats_out, scratch, scratch_bytes, a))
    return rc;
  return ppo_loss_launch(KL, a, stats_out, (hipStream_t)stream);
}

int skyjo_vec_ppo_loss(const float *logits, const float *log_mask, const float *value, const int64_t *actions, const float *logp_old,
                       const float *advantages, const float *value_targets, const float *values_old, int64_t m, float clip,
                       float vf_coef, float ent_coef, float vf_clip, float *grad_logits_out, float *grad_value_out, double *stats_out,
                       void *scratch, int64_t scratch_bytes, void *stream) {
  return ppo_loss("skyjo_vec_ppo_loss", false, logits, log_mask, nullptr, value, actions, logp_old, advantages, value_targets, values_old, m,
                         clip, vf_coef, ent_coef, vf_clip, 0.f, grad_logits_out, grad_value_out, stats_out, scratch, scratch_bytes, stream);
}

int skyjo_vec_ppo_loss_kl(const float *logits, const float *log_mask, const float *old_logits, const float *value, const int64_t *actions,
                          const float *logp_old, const float *advantages, const float *value_targets, const float *values_old, int64_t m,
                          float clip, float vf_coef, float ent_coef, float vf_clip, float kl_coeff, float *grad_logits_out,
                          float *grad_value_out, double *stats_out, void *scratch, int64_t scratch_bytes, void *stream) {
  return ppo_loss("skyjo_vec_ppo_loss_kl", true, logits, log_mask, old_logits, value, actions, logp_old, advantages, value_targets,
                        values_old, m, clip, vf_coef, ent_coef, vf_clip, kl_coeff, grad_logits_out, grad_value_out, stats_out, scratch,
                        scratch_bytes, stream);
}

// ---- a branch's training forward and backward on its float32 parameters (include/skyjo_vec.h: skyjo_vec_mlp_train_* for 1 .. 31
// inputs, skyjo_train.h; skyjo_vec_mlp_train_wide_* for 32 .. 163, skyjo_train_wide.h).  Every width has one implementation: `wide`
// below says which pair of entries the caller is (or, in skyjo_vec_ppo_update, which the engine's observation needs) ----
namespace {

constexpr int64_t kTrainMaxRows = (int64_t)1 << 30;
int64_t train_chunks(int64_t m) { return (m + SKT_CHUNK_ROWS - 1) / SKT_CHUNK_ROWS; }
bool train_is_wide(int D) { return D > SKT_IN - 1; }

// the checks the two calls share and the workspace's views; 0 or the code fail() returned
int train_args(const char *who, bool wide, int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, int64_t m,
               void *workspace, int64_t workspace_bytes, SkTrainArgs &a) {
  const std::string name(who);
  if (!params || !x || !workspace) return fail(SKYJO_E_INVALID, name + ": null argument");
  for (int i = 0; i < 6; i++)
    if (!params[i]) return fail(SKYJO_E_INVALID, name + ": null parameter");
  if (wide) {
    if (obs_dim < SKTW_MIN_IN || obs_dim > SKTW_MAX_IN || out_dim < 1 || out_dim > SKT_OUT)
      return fail(SKYJO_E_INVALID, name + ": obs_dim must be 32..163 and out_dim 1..32");
  } else if (obs_dim < 1 || obs_dim > SKT_IN - 1 || out_dim < 1 || out_dim > SKT_OUT) {
    return fail(SKYJO_E_INVALID, name + ": obs_dim must be 1..31 and out_dim 1..32");
  }
  if (m < 1 || m > kTrainMaxRows) return fail(SKYJO_E_INVALID, name + ": m must be at least 1");
  if (wide) {
    if (workspace_bytes < skyjo_vec_mlp_train_wide_workspace_bytes(obs_dim, out_dim, m))
      return fail(SKYJO_E_INVALID, name + ": workspace is smaller than skyjo_vec_mlp_train_wide_workspace_bytes");
  } else if (workspace_bytes < skyjo_vec_mlp_train_workspace_bytes(obs_dim, out_dim, m)) {
    return fail(SKYJO_E_INVALID, name + ": workspace is smaller than skyjo_vec_mlp_train_workspace_bytes");
  }
  if (!aligned16(params[2]) || !aligned16(params[4]) || !aligned16(workspace))
    return fail(SKYJO_E_INVALID, name + ": w2, w3 and workspace must be 16-byte aligned");
  for (int i = 0; i < 6; i++)
    if ((uintptr_t)params[i] & 3) return fail(SKYJO_E_INVALID, name + ": a parameter is not aligned to its element size");
  if ((uintptr_t)x & 3) return fail(SKYJO_E_INVALID, name + ": x is not aligned to its element size");
  a.w1 = params[0], a.b1 = params[1], a.w2 = params[2], a.b2 = params[3], a.w3 = params[4], a.b3 = params[5];
  a.x = x, a.m = m, a.D = obs_dim, a.O = out_dim, a.chunks = (int)train_chunks(m);
  const size_t act = (size_t)m * SKT_H;
  a.h1 = (float *)workspace, a.h2 = a.h1 + act, a.dz2 = a.h2 + act, a.dz1 = a.dz2 + act, a.part = a.dz1 + act;
  return SKYJO_OK;
}

}  // namespace

int64_t skyjo_vec_mlp_train_workspace_bytes(int32_t obs_dim, int32_t out_dim, int64_t m) {
  if (obs_dim < 1 || obs_dim > SKT_IN - 1 || out_dim < 1 || out_dim > SKT_OUT || m < 1 || m > kTrainMaxRows) return 0;
  return (int64_t)sizeof(float) * (4 * m * SKT_H + train_chunks(m) * SKT_PART);
}

int64_t skyjo_vec_mlp_train_wide_workspace_bytes(int32_t obs_dim, int32_t out_dim, int64_t m) {
  if (obs_dim < SKTW_MIN_IN || obs_dim > SKTW_MAX_IN || out_dim < 1 || out_dim > SKT_OUT || m < 1 || m > kTrainMaxRows) return 0;
  return (int64_t)sizeof(float) * (4 * m * SKT_H + train_chunks(m) * sktw_part(sktw_k(obs_dim)));
}

// the two calls and skyjo_vec_ppo_update: the checks and the kernels' arguments, nothing launched - and the launches
static int train_forward_check(const char *who, bool wide, int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, int64_t m, float *out,
                               void *workspace, int64_t workspace_bytes, SkTrainArgs &a) {
  if (!out) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if (int rc = train_args(who, wide, obs_dim, out_dim, params, x, m, workspace, workspace_bytes, a)) return rc;
  if ((uintptr_t)out & 3) return fail(SKYJO_E_INVALID, std::string(who) + ": out is not aligned to its element size");
  a.out = out;
  return SKYJO_OK;
}
static int train_forward_launch(const SkTrainArgs &a, hipStream_t s) {
  const unsigned tiles = (unsigned)((a.m + SKT_TILE_ROWS - 1) / SKT_TILE_ROWS);
  if (train_is_wide(a.D)) hipLaunchKernelGGL(k_mlp_train_wide_fwd, dim3(tiles), dim3(SKT_THREADS), 0, s, a);
  else hipLaunchKernelGGL(k_mlp_train_fwd, dim3(tiles), dim3(SKT_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int skyjo_vec_mlp_train_forward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, int64_t m, float *out,
                                void *workspace, int64_t workspace_bytes, void *stream) {
  SkTrainArgs a{};
  if (int rc = train_forward_check("skyjo_vec_mlp_train_forward", false, obs_dim, out_dim, params, x, m, out, workspace, workspace_bytes, a)) return rc;
  return train_forward_launch(a, (hipStream_t)stream);
}

int skyjo_vec_mlp_train_wide_forward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, int64_t m, float *out,
                                     void *workspace, int64_t workspace_bytes, void *stream) {
  SkTrainArgs a{};
  if (int rc = train_forward_check("skyjo_vec_mlp_train_wide_forward", true, obs_dim, out_dim, params, x, m, out, workspace, workspace_bytes, a))
    return rc;
  return train_forward_launch(a, (hipStream_t)stream);
}

static int train_backward_check(const char *who, bool wide, int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, const float *grad_out,
                                int64_t m, float *const grads[6], void *workspace, int64_t workspace_bytes, SkTrainArgs &a) {
  if (!grad_out || !grads) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  for (int i = 0; i < 6; i++)
    if (!grads[i]) return fail(SKYJO_E_INVALID, std::string(who) + ": null gradient");
  if (int rc = train_args(who, wide, obs_dim, out_dim, params, x, m, workspace, workspace_bytes, a)) return rc;
  if ((uintptr_t)grad_out & 3) return fail(SKYJO_E_INVALID, std::string(who) + ": grad_out is not aligned to its element size");
  for (int i = 0; i < 6; i++) {
    if ((uintptr_t)grads[i] & 3) return fail(SKYJO_E_INVALID, std::string(who) + ": a gradient is not aligned to its element size");
    a.grads[i] = grads[i];
  }
  a.g = grad_out;
  return SKYJO_OK;
}
static int train_backward_launch(const SkTrainArgs &a, hipStream_t s) {
  const unsigned tiles = (unsigned)((a.m + SKT_TILE_ROWS - 1) / SKT_TILE_ROWS);
  hipLaunchKernelGGL(k_mlp_train_bwd_rows, dim3(tiles), dim3(SKT_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  if (train_is_wide(a.D)) {  // (the row pass reads neither x nor W1: it is the narrow nets')
    hipLaunchKernelGGL(k_mlp_train_wide_bwd_weights, dim3((unsigned)a.chunks, SKT_SLICES), dim3(SKT_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_mlp_train_wide_bwd_finish, dim3((sktw_part(sktw_k(a.D)) + SKT_THREADS - 1) / SKT_THREADS), dim3(SKT_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    return SKYJO_OK;
  }
  hipLaunchKernelGGL(k_mlp_train_bwd_weights, dim3((unsigned)a.chunks, SKT_SLICES), dim3(SKT_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_mlp_train_bwd_finish, dim3((SKT_PART + SKT_THREADS - 1) / SKT_THREADS), dim3(SKT_THREADS), 0, s, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int skyjo_vec_mlp_train_backward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, const float *grad_out,
                                 int64_t m, float *const grads[6], void *workspace, int64_t workspace_bytes, void *stream) {
  SkTrainArgs a{};
  if (int rc = train_backward_check("skyjo_vec_mlp_train_backward", false, obs_dim, out_dim, params, x, grad_out, m, grads, workspace, workspace_bytes, a))
    return rc;
  return train_backward_launch(a, (hipStream_t)stream);
}

int skyjo_vec_mlp_train_wide_backward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, const float *grad_out,
                                      int64_t m, float *const grads[6], void *workspace, int64_t workspace_bytes, void *stream) {
  SkTrainArgs a{};
  if (int rc = train_backward_check("skyjo_vec_mlp_train_wide_backward", true, obs_dim, out_dim, params, x, grad_out, m, grads, workspace,
                                    workspace_bytes, a))
    return rc;
  return train_backward_launch(a, (hipStream_t)stream);
}

// ---- an epoch's order and a whole PPO update behind one call (include/skyjo_vec.h: skyjo_vec_rollout_shuffle, skyjo_vec_ppo_update;
// the kernels of their own: skyjo_epoch.h; every stage through the launchers above) ----
namespace {

int shuffle_check(const char *who, const int64_t *index, int64_t count, const int64_t *order_out, const int64_t *fault_out) {
  const std::string name(who);
  if (!index || !order_out || !fault_out) return fail(SKYJO_E_INVALID, name + ": null argument");
  if (count < 0 || count > SKE_MAX_COUNT) return fail(SKYJO_E_INVALID, name + ": count must lie in 0 .. 2^30");
  if ((((uintptr_t)index | (uintptr_t)order_out | (uintptr_t)fault_out) & 7) != 0)
    return fail(SKYJO_E_INVALID, name + ": index, order_out and fault_out must be 8-byte aligned");
  if (index == order_out || (index < order_out ? index + count > order_out : order_out + count > index))
    return fail(SKYJO_E_INVALID, name + ": order_out must not alias index");
  return SKYJO_OK;
}

// the order of (seed, epoch) and the count of its capped walks, on the current device; count == 0 writes the zero count alone
int shuffle_launch(const int64_t *index, int64_t count, uint64_t seed, uint32_t epoch, int64_t *order_out, int64_t *fault_out, hipStream_t s) {
  if (count > 0) {
    SkOrderArgs a{};
    ske_plan(seed, epoch, count, a);
    a.index = (const long long *)index, a.order = (long long *)order_out;
    hipLaunchKernelGGL(k_epoch_order, dim3((unsigned)((count + SKE_ORDER_THREADS - 1) / SKE_ORDER_THREADS)), dim3(SKE_ORDER_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_epoch_faults, dim3(1), dim3(SKE_FAULT_THREADS), 0, s, (const long long *)order_out, (long long)count, (long long *)fault_out);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

// skyjo_vec_ppo_update's workspace: every piece at a multiple of 256 bytes (the twelve gradients 16-byte aligned, as skyjo_vec_grad_norm's
// order of additions has torch's allocations).  R = max(min(minibatch, count), 1) rows; every size grows with count
struct UpdLayout {
  size_t obs, logmask, actions, logp, adv, vt, val, seats, old_logits, ws[2], out[2], g_logits, g_value, loss_stats, loss_scratch, grads[2][SKU_TENSORS],
      pair, order, acc, fault, total;
  int64_t ws_bytes[2], loss_scratch_bytes, rows;
};
constexpr int kUpdOut[2] = {SKYJO_NUM_ACTIONS, 1};  // the policy branch's outputs and the value branch's

UpdLayout upd_layout(int D, int64_t count, int64_t minibatch, bool kl) {
  UpdLayout u{};
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += (bytes + 255) & ~(size_t)255;
    return here;
  };
  const int64_t R = u.rows = std::max<int64_t>(std::min(minibatch, count), 1);
  const size_t f = sizeof(float);
  u.obs = take(R * D * f), u.logmask = take(R * SKYJO_NUM_ACTIONS * f), u.actions = take(R * sizeof(int64_t));
  u.logp = take(R * f), u.adv = take(R * f), u.vt = take(R * f), u.val = take(R * f), u.seats = take(R);
  u.old_logits = take(kl ? R * SKYJO_NUM_ACTIONS * f : 0);
  for (int b = 0; b < 2; b++) {
    u.ws_bytes[b] = train_is_wide(D) ? skyjo_vec_mlp_train_wide_workspace_bytes(D, kUpdOut[b], R) : skyjo_vec_mlp_train_workspace_bytes(D, kUpdOut[b], R);
    u.ws[b] = take((size_t)u.ws_bytes[b]), u.out[b] = take(R * kUpdOut[b] * f);
  }
  u.g_logits = take(R * SKYJO_NUM_ACTIONS * f), u.g_value = take(R * f), u.loss_stats = take(SK_LOSS_KL_STATS * sizeof(double));
  u.loss_scratch_bytes = loss_scratch_bytes(R, kl ? SK_LOSS_KL_STATS : SK_LOSS_STATS);
  u.loss_scratch = take((size_t)u.loss_scratch_bytes);
  for (int b = 0; b < 2; b++)
    for (int i = 0; i < SKU_TENSORS; i++) u.grads[b][i] = take(sku_tensor_elems(i, D, kUpdOut[b]) * f);
  u.pair = take(2 * f), u.order = take((size_t)count * sizeof(int64_t)), u.acc = take(SKE_ACC * sizeof(double)), u.fault = take(sizeof(int64_t));
  u.total = at;
  return u;
}

bool upd_sizes_valid(int64_t count, int64_t minibatch) { return count >= 0 && count <= SKE_MAX_COUNT && minibatch >= 1; }

// the arguments of the stages whose views depend on the slice's row count m: both branches' forward and backward, and the head
struct UpdSlice {
  SkTrainArgs fwd[2], bwd[2];
  SkLossArgs loss;
};

}  // namespace

int skyjo_vec_rollout_shuffle(const int64_t *index, int64_t count, uint64_t seed, uint32_t epoch, int64_t *order_out, int64_t *fault_out,
                              void *stream) {
  if (int rc = shuffle_check("skyjo_vec_rollout_shuffle", index, count, order_out, fault_out)) return rc;
  return shuffle_launch(index, count, seed, epoch, order_out, fault_out, (hipStream_t)stream);
}

int64_t skyjo_vec_ppo_update_workspace_bytes(const skyjo_vec *h, int64_t count, int64_t minibatch, int32_t with_kl) {
  if (!h || !upd_sizes_valid(count, minibatch)) return 0;
  return (int64_t)upd_layout(sk_engine_view(h).L->D, count, minibatch, with_kl != 0).total;
}

int skyjo_vec_ppo_update(skyjo_vec *h, const skyjo_vec_ppo_update_args *a, void *workspace, int64_t workspace_bytes, double *epoch_stats_out,
                         int64_t *fault_out, void *stream) {
  static const char *who = "skyjo_vec_ppo_update";
  const std::string name(who);
  // ---- every check of every stage, before the first launch: an update runs whole or not at all ----
  if (!h || !a || !workspace || !epoch_stats_out || !fault_out) return fail(SKYJO_E_INVALID, name + ": null argument");
  if (!a->policy_net || !a->value_net || !a->policy_state || !a->value_state) return fail(SKYJO_E_INVALID, name + ": null net or Adam state");
  if (a->epochs < 1 || a->minibatch < 1 || a->first_step < 1) return fail(SKYJO_E_INVALID, name + ": epochs, minibatch and first_step must be at least 1");
  if (!upd_sizes_valid(a->count, a->minibatch)) return fail(SKYJO_E_INVALID, name + ": count must lie in 0 .. 2^30");
  if (a->T < 1 || a->value_stride < 1) return fail(SKYJO_E_INVALID, name + ": T and value_stride must be at least 1");
  if (int rc = check_layout(a->layout)) return rc;
  const SkEngineView e = sk_engine_view(h);
  const int D = e.L->D;
  const int64_t n_rows = (int64_t)a->T * e.B, count = a->count, mb = a->minibatch;
  if (count > n_rows) return fail(SKYJO_E_INVALID, name + ": count exceeds T * num_envs");
  if ((((uintptr_t)epoch_stats_out | (uintptr_t)fault_out | (uintptr_t)a->index | (uintptr_t)a->orders) & 7) != 0)
    return fail(SKYJO_E_INVALID, name + ": epoch_stats_out, fault_out, index and orders must be 8-byte aligned");
  if (!aligned16(workspace)) return fail(SKYJO_E_INVALID, name + ": workspace must be 16-byte aligned");
  skyjo_vec_mlp *const nets[2] = {a->policy_net, a->value_net};
  for (int b = 0; b < 2; b++)
    if (nets[b]->device_id != e.device_id || nets[b]->obs_dim != D || nets[b]->out_dim != kUpdOut[b])
      return fail(SKYJO_E_INVALID, name + ": the nets must live on the engine's device, take the engine's observation and have 26 outputs and 1");
  const bool kl = a->behaviour != nullptr;
  const bool clipping = a->max_grad_norm > 0.f;  // (<= 0 and NaN: no clipping; +inf: measure only)
  const UpdLayout u = upd_layout(D, count, mb, kl);
  if (workspace_bytes < (int64_t)u.total) return fail(SKYJO_E_INVALID, name + ": workspace is smaller than skyjo_vec_ppo_update_workspace_bytes");
  uint8_t *const w = (uint8_t *)workspace;
  auto F = [&](size_t off) { return (float *)(w + off); };
  int64_t *const ws_order = (int64_t *)(w + u.order), *const ws_fault = (int64_t *)(w + u.fault);
  double *const loss_stats = (double *)(w + u.loss_stats);
  float *const pair = F(u.pair);
  float *const *const params[2] = {a->policy_params, a->value_params};
  void *const state[2] = {a->policy_state, a->value_state};
  const int64_t state_bytes[2] = {a->policy_state_bytes, a->value_state_bytes};
  float *grads[2][SKU_TENSORS];
  const float *twelve[2 * SKU_TENSORS];
  int64_t counts[2 * SKU_TENSORS];
  for (int b = 0; b < 2; b++)
    for (int i = 0; i < SKU_TENSORS; i++) {
      grads[b][i] = F(u.grads[b][i]);
      twelve[b * SKU_TENSORS + i] = grads[b][i], counts[b * SKU_TENSORS + i] = (int64_t)sku_tensor_elems(i, D, kUpdOut[b]);
    }
  // the selection and the schedule
  const int64_t *const order0 = a->orders ? a->orders : ws_order;
  if (!a->orders)
    if (int rc = shuffle_check(who, a->index, count, ws_order, ws_fault)) return rc;
  SkGatherArgs gather{};
  if (int rc = gather_check(who, h, a->records, a->layout, a->T, order0, std::min(mb, count), a->actions, a->logp, a->values, a->value_stride,
                            a->advantages, a->value_targets, a->adv_mean, a->adv_std, F(u.obs), F(u.logmask), (int64_t *)(w + u.actions), F(u.logp),
                            F(u.adv), F(u.vt), F(u.val), w + u.seats, gather))
    return rc;
  if (kl)
    if (int rc = gather_logits_check(who, a->behaviour, n_rows, order0, std::min(mb, count), F(u.old_logits))) return rc;
  // the optimiser: both branches' Adam at the first step (a later step changes the scalars alone) and the norm over the twelve gradients
  SkUpdArgs adam[2];
  SkNormArgs norm{};
  for (int b = 0; b < 2; b++) {
    adam[b] = SkUpdArgs{};
    if (int rc = adam_check(who, nets[b], params[b], grads[b], state[b], state_bytes[b], a->lr, a->beta1, a->beta2, a->eps, a->first_step,
                            clipping ? pair + 1 : nullptr, adam[b]))
      return rc;
  }
  if (clipping)
    if (int rc = grad_norm_check(who, twelve, counts, 2 * SKU_TENSORS, a->max_grad_norm, pair, norm)) return rc;
  // the stages whose views depend on the row count: a full slice, and the short last one where count is no multiple of minibatch
  const int64_t steps = (count + mb - 1) / mb, rows[2] = {std::min(mb, count), count % mb};
  UpdSlice slice[2];
  for (int k = 0; k < 2; k++) {
    const int64_t m = rows[k];
    if (m == 0) continue;  // (count == 0, or no short slice)
    UpdSlice &sl = slice[k];
    sl = UpdSlice{};
    for (int b = 0; b < 2; b++) {
      if (int rc = train_forward_check(who, train_is_wide(D), D, kUpdOut[b], params[b], F(u.obs), m, F(u.out[b]), w + u.ws[b], u.ws_bytes[b], sl.fwd[b])) return rc;
      if (int rc = train_backward_check(who, train_is_wide(D), D, kUpdOut[b], params[b], F(u.obs), b == 0 ? F(u.g_logits) : F(u.g_value), m, grads[b], w + u.ws[b],
                                        u.ws_bytes[b], sl.bwd[b]))
        return rc;
    }
    if (int rc = ppo_loss_check(who, kl, F(u.out[0]), F(u.logmask), kl ? F(u.old_logits) : nullptr, F(u.out[1]), (const int64_t *)(w + u.actions),
                                F(u.logp), F(u.adv), F(u.vt), F(u.val), m, a->clip, a->vf_coef, a->ent_coef, a->vf_clip, kl ? a->kl_coeff : 0.f,
                                F(u.g_logits), F(u.g_value), loss_stats, w + u.loss_scratch, u.loss_scratch_bytes, sl.loss))
      return rc;
  }
  // ---- the launches: nothing below allocates, copies to the host, synchronises or looks at device data ----
  DevGuard guard_(e.device_id);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(epoch_stats_out, 0, (size_t)a->epochs * SKYJO_UPDATE_STATS * sizeof(double), s));
  HIPCHK(hipMemsetAsync(fault_out, 0, sizeof(int64_t), s));
  if (count == 0) return SKYJO_OK;
  SkStatsArgs st{};
  st.stats = loss_stats, st.pair = clipping ? pair : nullptr, st.acc = (double *)(w + u.acc);
  st.epoch_fault = a->orders ? nullptr : (const long long *)ws_fault, st.fault_out = (long long *)fault_out;
  st.inv_seen = 1.0 / (double)count, st.inv_steps = 1.0 / (double)steps, st.ns = kl ? SK_LOSS_KL_STATS : SK_LOSS_STATS;
  int64_t step = a->first_step;
  for (int32_t ep = 0; ep < a->epochs; ep++) {
    const int64_t *order = a->orders ? a->orders + (size_t)ep * count : ws_order;
    if (!a->orders)
      if (int rc = shuffle_launch(a->index, count, a->seed, (uint32_t)ep, ws_order, ws_fault, s)) return rc;
    for (int64_t k = 0; k < steps; k++, step++) {
      const int64_t m = std::min(mb, count - k * mb);
      const UpdSlice &sl = slice[m == rows[0] ? 0 : 1];
      gather.index = (const long long *)(order + k * mb), gather.m = m;
      if (int rc = gather_launch(gather, s)) return rc;
      if (kl)
        if (int rc = gather_logits_launch(a->behaviour, n_rows, order + k * mb, m, F(u.old_logits), s)) return rc;
      for (int b = 0; b < 2; b++)
        if (int rc = train_forward_launch(sl.fwd[b], s)) return rc;
      if (int rc = ppo_loss_launch(kl, sl.loss, loss_stats, s)) return rc;
      for (int b = 0; b < 2; b++)
        if (int rc = train_backward_launch(sl.bwd[b], s)) return rc;
      if (clipping)
        if (int rc = grad_norm_launch(norm, s)) return rc;
      for (int b = 0; b < 2; b++) {
        adam_scalars(adam[b], a->lr, a->beta1, a->beta2, a->eps, step);
        if (int rc = adam_launch(nets[b], adam[b], s)) return rc;
      }
      st.m = (double)m, st.first = k == 0, st.last = k == steps - 1, st.row = epoch_stats_out + (size_t)ep * SKYJO_UPDATE_STATS;
      hipLaunchKernelGGL(k_update_stats, dim3(1), dim3(64), 0, s, st);
      HIPCHK(hipGetLastError());
    }
  }
  return SKYJO_OK;
}

// ---- arena rollouts: a policy per seat, and the episode-end columns as per-seat results (include/skyjo_vec.h: skyjo_vec_arena_*,
// skyjo_vec_episode_stats; the kernels: skyjo_arena.h).  The engine is stepped through the public skyjo_vec_step_collect. ----
namespace {

struct ArenaPlan {
  SkArenaArgs a{};
  const skyjo_vec_mlp *net[SKYJO_MAX_PLAYERS] = {};   // the distinct policy nets, in the order of their first seat
  const skyjo_vec_mlp *vnet[SKYJO_MAX_PLAYERS] = {};  // the distinct value nets, likewise
  int vnets = 0;
  bool act = false;  // value nets were given (skyjo_vec_arena_act / _collect): k_arena<true>
  SkEngineView e{};
};

int64_t arena_act_bytes(int32_t B, int nets, int vnets) {
  return ((int64_t)nets * sk_arena_slice(B) + (int64_t)vnets * sk_arena_vslice(B)) * (int64_t)sizeof(float);
}

// the seats and the value nets (null: none, the plan of skyjo_vec_arena_select / _rollout) checked against the engine, the distinct
// nets of either kind and the workspace - the policy slices, then the value slices; 0 or the code fail() returned
int arena_plan(const char *who, const skyjo_vec *h, const skyjo_vec_seat_policy *seats, const skyjo_vec_mlp *const *value_nets, void *workspace,
               int64_t workspace_bytes, ArenaPlan &p) {
  const std::string name(who);
  if (!h || !seats) return fail(SKYJO_E_INVALID, name + ": null argument");
  p.e = sk_engine_view(h);
  p.act = value_nets != nullptr;
  const SkLayout &L = *p.e.L;
  static_assert(SKYJO_MAX_PLAYERS <= 16, "a seat's net is a 4-bit field of SkArenaArgs::seat_net, its kind a 2-bit field of ::kinds");
  SkArenaArgs &a = p.a;
  for (int s = 0; s < L.N; s++) {
    const skyjo_vec_mlp *m = seats[s].net;
    const int32_t kind = seats[s].kind;
    if (kind != SKYJO_SEAT_SAMPLE && kind != SKYJO_SEAT_GREEDY && kind != SKYJO_SEAT_RANDOM) return fail(SKYJO_E_INVALID, name + ": unknown seat kind");
    if (kind == SKYJO_SEAT_RANDOM) {
      if (m) return fail(SKYJO_E_INVALID, name + ": a SKYJO_SEAT_RANDOM seat takes no net");
    } else {
      if (!m) return fail(SKYJO_E_INVALID, name + ": a SKYJO_SEAT_SAMPLE or SKYJO_SEAT_GREEDY seat needs a net");
      if (m->net.out_dim != SKYJO_NUM_ACTIONS) return fail(SKYJO_E_INVALID, name + ": a seat's net needs 26 outputs");
      if (m->device_id != p.e.device_id || m->obs_dim != L.D)
        return fail(SKYJO_E_INVALID, name + ": a seat's net must live on the engine's device and take the engine's observation");
      int j = 0;
      while (j < a.nets && p.net[j] != m) j++;
      if (j == a.nets) p.net[a.nets++] = m;
      a.seat_net |= (uint64_t)j << (4 * s);
    }
    a.kinds |= (uint32_t)kind << (2 * s);
  }
  for (int s = 0; p.act && s < L.N; s++) {
    const skyjo_vec_mlp *m = value_nets[s];
    int j = (int)SK_ARENA_NO_VNET;
    if (m) {
      if (m->net.out_dim != 1) return fail(SKYJO_E_INVALID, name + ": a seat's value net needs 1 output");
      if (m->device_id != p.e.device_id || m->obs_dim != L.D)
        return fail(SKYJO_E_INVALID, name + ": a seat's value net must live on the engine's device and take the engine's observation");
      for (j = 0; j < p.vnets && p.vnet[j] != m; j++) {}
      if (j == p.vnets) p.vnet[p.vnets++] = m;
    }
    a.seat_vnet |= (uint64_t)j << (4 * s);
  }
  if (a.nets + p.vnets) {
    if (!workspace) return fail(SKYJO_E_INVALID, name + ": seats with nets need a workspace");
    if ((uintptr_t)workspace & 15) return fail(SKYJO_E_INVALID, name + ": workspace must be 16-byte aligned");
    if (workspace_bytes < arena_act_bytes(p.e.B, a.nets, p.vnets))
      return fail(SKYJO_E_INVALID,
                  name + ": workspace is smaller than " + (p.act ? "skyjo_vec_arena_act_workspace_bytes" : "skyjo_vec_arena_workspace_bytes"));
    a.logits = (const float *)workspace;
    a.values = a.logits + (size_t)a.nets * sk_arena_slice(p.e.B);
  }
  a.n = p.e.B, a.game_id0 = p.e.game_id0, a.Dp = L.Dp, a.rec_bytes = L.rec_bytes, a.N = L.N;
  return SKYJO_OK;
}

// one lockstep iteration: a full-batch forward per distinct policy net (none when actions is null: the values only) and per distinct
// value net, then ONE k_arena.  logp and values_out: with value nets only
int arena_launch(const ArenaPlan &p, const uint8_t *rec, int planar, uint64_t seed, uint64_t ticket, int32_t *actions, float *logp, float *values_out,
                 hipStream_t s) {
  SkArenaArgs a = p.a;
  a.rec = rec, a.planar = planar, a.seed = seed, a.ticket = ticket, a.actions = actions, a.logp = logp, a.values_out = values_out;
  const SkMlpDraw nodraw{};
  auto forward = [&](const skyjo_vec_mlp *m, const float *out) {
    return launch_mlp(m, m, 1, rec, (int)a.rec_bytes, m->obs_dim, (int64_t)a.n, const_cast<float *>(out), nodraw, nullptr, s, planar);
  };
  for (int j = 0; actions && j < a.nets; j++)
    if (int rc = forward(p.net[j], a.logits + (size_t)j * sk_arena_slice(a.n))) return rc;
  for (int j = 0; j < p.vnets; j++)
    if (int rc = forward(p.vnet[j], a.values + (size_t)j * sk_arena_vslice(a.n))) return rc;
  const dim3 grid((unsigned)((a.n + SK_ARENA_BLOCK - 1) / SK_ARENA_BLOCK)), block(SK_ARENA_BLOCK);
  if (p.act) hipLaunchKernelGGL(k_arena<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_arena<false>, grid, block, 0, s, a);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

// T iterations, each arena_launch on records[t] and skyjo_vec_step_collect into records[t + 1]; with value nets logp and values are
// recorded too and one more launch, the values only, reads the records the rollout ends on
int arena_iterate(skyjo_vec *h, const ArenaPlan &p, int32_t T, uint64_t seed, uint64_t first_ticket, const skyjo_vec_rollout_buffers *b, void *stream) {
  int64_t lay = 0;  // what skyjo_vec_step_collect writes: tile-planar records with SKYJO_REC_TILE_PLANAR_ALL, row-major otherwise
  if (int rc = skyjo_vec_get_option(h, SKYJO_OPT_RECORD_LAYOUT, &lay)) return rc;
  const int planar = lay == SKYJO_REC_TILE_PLANAR_ALL;
  const size_t B = (size_t)p.e.B, N = (size_t)p.e.L->N, per_it = (planar ? p.e.G : B) * (size_t)p.e.L->rec_bytes;
  uint8_t *rec = (uint8_t *)b->records;
  for (int t = 0; t < T + (p.act ? 1 : 0); t++) {
    const bool acting = t < T;
    int32_t *act = acting ? b->actions + (size_t)t * B : nullptr;
    {
      DevGuard guard_(p.e.device_id);
      if (int rc = arena_launch(p, rec + (size_t)t * per_it, planar, seed, first_ticket + (uint64_t)t, act, p.act && acting ? b->logp + (size_t)t * B : nullptr,
                                p.act ? b->values + (size_t)t * B : nullptr, (hipStream_t)stream))
        return rc;
    }
    if (acting)
      if (int rc = skyjo_vec_step_collect(h, act, rec + (size_t)(t + 1) * per_it, b->final_rewards + (size_t)t * B * N, b->episode_end + (size_t)t * B, stream))
        return rc;
  }
  return SKYJO_OK;
}

constexpr int64_t kStatMaxRows = (int64_t)SK_STAT_ROWS << 30;

}  // namespace

int64_t skyjo_vec_arena_workspace_bytes(const skyjo_vec *h, int32_t distinct_nets) {
  if (!h || distinct_nets < 0 || distinct_nets > SKYJO_MAX_PLAYERS) return 0;
  return arena_act_bytes(sk_engine_view(h).B, distinct_nets, 0);
}

int64_t skyjo_vec_arena_act_workspace_bytes(const skyjo_vec *h, int32_t distinct_policy_nets, int32_t distinct_value_nets) {
  if (!h || distinct_policy_nets < 0 || distinct_policy_nets > SKYJO_MAX_PLAYERS || distinct_value_nets < 0 || distinct_value_nets > SKYJO_MAX_PLAYERS)
    return 0;
  return arena_act_bytes(sk_engine_view(h).B, distinct_policy_nets, distinct_value_nets);
}

int skyjo_vec_arena_select(skyjo_vec *h, const skyjo_vec_seat_policy *seats, const void *records, int32_t layout, uint64_t seed, uint64_t ticket,
                           int32_t *actions_out, void *workspace, int64_t workspace_bytes, void *stream) {
  static const char *who = "skyjo_vec_arena_select";
  if (!records || !actions_out) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if (int rc = check_layout(layout)) return rc;
  ArenaPlan p;
  if (int rc = arena_plan(who, h, seats, nullptr, workspace, workspace_bytes, p)) return rc;
  DevGuard guard_(p.e.device_id);
  return arena_launch(p, (const uint8_t *)records, (int)(layout == SKYJO_REC_TILE_PLANAR), seed, ticket, actions_out, nullptr, nullptr, (hipStream_t)stream);
}

int skyjo_vec_arena_rollout(skyjo_vec *h, const skyjo_vec_seat_policy *seats, int32_t T, uint64_t seed, uint64_t first_ticket,
                            const skyjo_vec_rollout_buffers *b, void *workspace, int64_t workspace_bytes, void *stream) {
  static const char *who = "skyjo_vec_arena_rollout";
  if (!b || !b->records || !b->actions || !b->final_rewards || !b->episode_end) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if (b->logp || b->values) return fail(SKYJO_E_INVALID, std::string(who) + ": logp and values must be NULL (the arena writes neither)");
  if (T < 1) return fail(SKYJO_E_INVALID, std::string(who) + ": T must be at least 1");
  ArenaPlan p;
  if (int rc = arena_plan(who, h, seats, nullptr, workspace, workspace_bytes, p)) return rc;
  return arena_iterate(h, p, T, seed, first_ticket, b, stream);
}

int skyjo_vec_arena_act(skyjo_vec *h, const skyjo_vec_seat_policy *seats, const skyjo_vec_mlp *const *value_nets, const void *records, int32_t layout,
                        uint64_t seed, uint64_t ticket, int32_t *actions_out, float *logp_out, float *values_out, void *workspace,
                        int64_t workspace_bytes, void *stream) {
  static const char *who = "skyjo_vec_arena_act";
  if (!records || !values_out || !value_nets) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if ((actions_out == nullptr) != (logp_out == nullptr)) return fail(SKYJO_E_INVALID, std::string(who) + ": actions_out and logp_out go together");
  if (int rc = check_layout(layout)) return rc;
  ArenaPlan p;
  if (int rc = arena_plan(who, h, seats, value_nets, workspace, workspace_bytes, p)) return rc;
  DevGuard guard_(p.e.device_id);
  return arena_launch(p, (const uint8_t *)records, (int)(layout == SKYJO_REC_TILE_PLANAR), seed, ticket, actions_out, logp_out, values_out,
                      (hipStream_t)stream);
}

int skyjo_vec_arena_collect(skyjo_vec *h, const skyjo_vec_seat_policy *seats, const skyjo_vec_mlp *const *value_nets, int32_t T, uint64_t seed,
                            uint64_t first_ticket, const skyjo_vec_rollout_buffers *b, void *workspace, int64_t workspace_bytes, void *stream) {
  static const char *who = "skyjo_vec_arena_collect";
  if (!b || !b->records || !b->actions || !b->logp || !b->values || !b->final_rewards || !b->episode_end)
    return fail(SKYJO_E_INVALID, std::string(who) + ": null argument (every column of the buffers is required)");
  if (T < 1) return fail(SKYJO_E_INVALID, std::string(who) + ": T must be at least 1");
  if (!value_nets) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  ArenaPlan p;
  if (int rc = arena_plan(who, h, seats, value_nets, workspace, workspace_bytes, p)) return rc;
  return arena_iterate(h, p, T, seed, first_ticket, b, stream);
}

int64_t skyjo_vec_episode_stats_scratch_bytes(int64_t rows, int32_t num_players) {
  if (rows < 1 || rows > kStatMaxRows || num_players < 1 || num_players > SKYJO_MAX_PLAYERS) return 0;
  return (rows + SK_STAT_ROWS - 1) / SK_STAT_ROWS * (int64_t)((1 + 3 * num_players) * sizeof(double));
}

int skyjo_vec_episode_stats(const double *final_rewards, const uint8_t *episode_end, int64_t rows, int32_t num_players, double *stats_out,
                            void *scratch, int64_t scratch_bytes, void *stream) {
  static const char *who = "skyjo_vec_episode_stats";
  if (!final_rewards || !episode_end || !stats_out || !scratch) return fail(SKYJO_E_INVALID, std::string(who) + ": null argument");
  if (rows < 1 || rows > kStatMaxRows) return fail(SKYJO_E_INVALID, std::string(who) + ": rows must be at least 1");
  if (num_players < 1 || num_players > SKYJO_MAX_PLAYERS) return fail(SKYJO_E_INVALID, std::string(who) + ": num_players must lie in 1 .. 12");
  if ((((uintptr_t)final_rewards | (uintptr_t)stats_out | (uintptr_t)scratch) & 7) != 0)
    return fail(SKYJO_E_INVALID, std::string(who) + ": final_rewards, stats_out and scratch must be 8-byte aligned");
  if (scratch_bytes < skyjo_vec_episode_stats_scratch_bytes(rows, num_players))
    return fail(SKYJO_E_INVALID, std::string(who) + ": scratch is smaller than skyjo_vec_episode_stats_scratch_bytes");
  const int64_t nb = (rows + SK_STAT_ROWS - 1) / SK_STAT_ROWS;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_episode_stats, dim3((unsigned)nb), dim3(SK_STAT_THREADS), 0, s, final_rewards, episode_end, (long long)rows, (int)num_players,
                     (double *)scratch);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_episode_stats_finish, dim3(1), dim3(SK_STAT_FIN_THREADS), 0, s, (const double *)scratch, (int)nb, (int)num_players, stats_out);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

}  // extern "C"
