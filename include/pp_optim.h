/* pp_optim.h -- the optimizer entry points of libpp_hip.so (csrc/pp_optim.hip): one fused Adam step over a list of
 * f32 tensors, with optional global-norm clipping and an optional skip of a step whose gradients are not finite,
 * decided on the device.  The conventions of pp_hip.h hold: everything runs on `stream`, nothing allocates, copies
 * through a copy engine or synchronises, arguments are validated before any HIP call (PP_ERR_VALUE), one context per
 * stream.
 *
 * The optimizer is torch.optim.Adam with L2 weight_decay, amsgrad=False, maximize=False.
 *
 * Tensors.  Parameters and gradients are n_tensors separate f32 arrays; their addresses and sizes are HOST arrays
 * (p_ptrs, g_ptrs, numel), read during the call and passed on to the kernels by value, 128 tensors per launch (a
 * longer list takes several launches).  A pointer needs the alignment of a float; where both the parameter's and the
 * gradient's are 16-byte aligned the kernels move 16 bytes per lane.  numel 0 is allowed (its pointers are not read).
 * The two moments are FLAT f32 buffers, 16-byte aligned: tensor i starts at sum_{j<i} round_up(numel_j, 4) floats; the
 * pad floats are never read or written.  A flat gradient (pp_adam_pack_dev) has the same offsets, its pads are
 * written as 0, and is handed to pp_adam_step_dev as the table of its segments' addresses.
 *
 * state_dev: 64 bytes, 16-byte aligned, zeroed once by the caller, then owned by the library:
 *     int64 step;  int64 skipped;  double grad_norm;  40 bytes reserved (the call's scalars for the update kernel)
 * workspace_dev: pp_adam_workspace_bytes(n_tensors, numel) bytes, 8-byte aligned; read and written only when
 *     max_grad_norm > 0 or skip_nonfinite is set (may be NULL otherwise); its contents on entry do not matter.
 *
 * Arithmetic of one pp_adam_step_dev call (f32 unless stated; fma(a, b, c) = a*b + c with ONE rounding, every other
 * operation rounds by itself):
 *     t  = step + 1
 *     gs = f32(grad_scale)
 *     G  = sqrt(sum (g*gs)^2): each product rounded to f32, squared and summed in f64, in a fixed order (the result
 *          is bit-reproducible); computed only with clipping or skip_nonfinite on, and then grad_norm = G
 *     if skip_nonfinite and some g*gs is not finite: skipped += 1; p, m, v and step keep their bits
 *     otherwise step = t and
 *       clip = max_grad_norm > 0 ? min(1, max_grad_norm / (G + 1e-6)) : 1     (f64; NaN stays NaN, as torch's clamp)
 *       s    = f32(grad_scale * clip)                                          (the product in f64)
 *       bc1  = 1 - beta1^t,  bc2 = 1 - beta2^t                                 (f64)
 *       step_size = f32(lr / bc1),  r = f32(1 / sqrt(bc2))
 *       per element, with b2 = f32(beta2), c1 = f32(1 - beta1), c2 = f32(1 - beta2), wd = f32(weight_decay),
 *       e = f32(eps):
 *         g1 = s == 1 ? g : g*s
 *         g2 = wd == 0 ? g1 : fma(wd, p, g1)
 *         m' = fma(c1, g2 - m, m)
 *         v' = fma(c2*g2, g2, b2*v)
 *         p' = p - (step_size*m') / fma(sqrt(v'), r, e)
 * With both options off, NaN and Inf propagate as in torch: an element with a non-finite gradient becomes non-finite
 * and no other does.
 *
 * Launches, in stream order: per 128 tensors one k_adam_stats (only with clipping or skip_nonfinite), one
 * k_adam_prepare, per 128 tensors one k_adam_update; pp_adam_pack_dev is one k_adam_pack per 128 tensors.
 *
 * PP_ERR_VALUE: a NULL context, table, moment, params or state pointer; a NULL workspace when it is needed; n_tensors
 * outside 1..4096; a numel outside 0..2^31-1; a NULL or misaligned tensor pointer with numel > 0; misaligned flat
 * buffers, state or workspace; lr, eps or weight_decay negative or not finite; a beta outside [0, 1); grad_scale not
 * positive and finite; max_grad_norm NaN.  pp_adam_workspace_bytes returns the byte count (at least 16), or
 * PP_ERR_VALUE. */
#ifndef PP_OPTIM_H
#define PP_OPTIM_H

#include "pp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PP_ADAM_MAX_TENSORS 4096
#define PP_ADAM_STATE_BYTES 64

typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
  double grad_scale;     /* multiplies every gradient first (1 / world size); > 0 */
  double max_grad_norm;  /* <= 0: no clipping */
  int32_t skip_nonfinite, reserved;
} pp_adam_params_t;

int64_t pp_adam_workspace_bytes(int32_t n_tensors, const int64_t *numel);
int pp_adam_pack_dev(pp_ctx_t *ctx, void *stream, int32_t n_tensors, const float *const *g_ptrs,
                     const int64_t *numel, float *flat_g_dev);
int pp_adam_step_dev(pp_ctx_t *ctx, void *stream, int32_t n_tensors, float *const *p_ptrs,
                     const float *const *g_ptrs, const int64_t *numel, float *m_flat_dev, float *v_flat_dev,
                     const pp_adam_params_t *params, void *state_dev, void *workspace_dev);

#ifdef __cplusplus
}
#endif
#endif
