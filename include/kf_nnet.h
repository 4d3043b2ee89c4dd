/*
 * kf_nnet.h — C-ABI of this build's host layer: the C++ restatement of the
 * reference's Go packages internal/nnet (xconfig.go, layers.go, model.go,
 * forward.go, network_backward.go, train_step.go) and internal/gpu
 * (optimize.go), running on the MI355X kernels of kf_ops.h.
 *
 * The reference's host code is Go; no Go toolchain exists in this image, so the
 * host layer is C++. The entry points below are the
 * Network / Trainer API of internal/nnet flattened into C:
 *   nnet_create        <- BuildModelFromString (model.go:31) + NewNetwork (forward.go:111)
 *   nnet_forward       <- Network.Forward (forward.go:148)
 *   nnet_backward      <- Network.Backward (network_backward.go:94)
 *   nnet_sgd           <- SGDOptimizer.Update for every parameter (optimize.go:95)
 *   nnet_train_step    <- TrainStep (train_step.go:142) with the chain objective
 * Errors: NULL / -1 with the text in nnet_last_error() (thread-local).
 */
#ifndef KALDI_FP16_AMD_KF_NNET_H
#define KALDI_FP16_AMD_KF_NNET_H
#include <stddef.h>
#include <stdint.h>

#include "kf_ops.h" /* KfNgOpts */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct KfNet KfNet;

/* layer type codes reported by nnet_layer_info (xconfig.go:18-30 order) */
enum {
    NNET_INPUT = 0, NNET_IDCT, NNET_LINEAR, NNET_BATCHNORM, NNET_SPECAUGMENT,
    NNET_COMBINE_FEATURE_MAPS, NNET_CONV_RELU_BN, NNET_TDNNF, NNET_ATTENTION,
    NNET_PREFINAL, NNET_OUTPUT
};

const char *nnet_last_error(void);

/* parse + resolve an xconfig and allocate weights/activations for max_frames */
KfNet *nnet_create(const char *xconfig_text, int max_frames);
/* the same network without device storage (no GPU needed): layers, the flat
 * parameter layout and the data-parallel bucket plan can be queried; forward,
 * backward, sgd and the parameter setters fail on it. The MI355X kernels' shape
 * constraints (dims multiples of 8 / 32) are not enforced here. */
KfNet *nnet_create_layout(const char *xconfig_text, int max_frames);
/* parse + resolve only, no device work: "name type in out" per layer, then
 * "params N"; returns the bytes needed (incl. NUL) or -1 */
int nnet_parse_summary(const char *xconfig_text, char *out, int outlen);
void nnet_free(KfNet *net);

int nnet_num_layers(const KfNet *net);  /* excluding input layers */
int nnet_layer_info(const KfNet *net, int idx, char *name, int namelen, int *type, int *in_dim,
                    int *out_dim);
/* trainable parameters: flat fp32 master / fp16 working / fp32 grad / fp32 velocity */
long long nnet_num_params(const KfNet *net);
int nnet_num_param_tensors(const KfNet *net);
int nnet_param_info(const KfNet *net, int idx, char *name, int namelen, int *rows, int *cols,
                    long long *offset);
/* host fp32 values in the flat layout; stored fp16 by truncation
 * (internal/gpu/tensor.go:158-173) and the master copy = that fp16 value
 * (optimize.go:52-70 via ops_fp16_to_fp32) */
int nnet_set_params(KfNet *net, const float *host_flat);
int nnet_get_params(const KfNet *net, float *host_flat); /* fp32 master */
/* which = 0: the layer's (first) BatchNorm, 1: prefinal's second BatchNorm;
 * target_rms <= 0: the layer's configured target-rms (a batchnorm-component's, else 1) */
int nnet_set_bn(KfNet *net, const char *layer, int which, const float *mean, const float *var,
                const float *gamma, const float *beta, float eps, float target_rms);

/* replace an idct-layer's matrix: host fp32 [dim x dim], y = x . m (weight_loader.go:88-97) */
int nnet_set_idct(KfNet *net, const char *layer, const float *m, int rows, int cols);
/* attention layer key scale (> 0); default 1/sqrt(key-dim) or the xconfig key-scale */
int nnet_set_key_scale(KfNet *net, const char *layer, float key_scale);

/* forward with the ivector input (an input layer named "ivector", read through
 * ReplaceIndex(ivector, t, 0)): ivectors fp16 [B x ivector-dim] on the device, one row per
 * sequence; seq_row0 host int[B+1] with the frame offsets (0 ... T). */
int nnet_forward_ivector(KfNet *net, const void *features_dev, int T, const void *ivectors_dev, int B,
                         const int *seq_row0);
/* forward on T frames of fp16 features already in device memory */
int nnet_forward(KfNet *net, const void *features_dev, int T);
/* device pointer of a layer's output activation (fp16 [rows x cols]) */
const void *nnet_activation(const KfNet *net, const char *layer, int *rows, int *cols);
/* backward from the fp16 gradient of the chain output [T x num_pdfs] */
int nnet_backward(KfNet *net, const void *out_grad_dev);
/* Backward with two seeds (Kaldi's chain xent-regularize): out_grad_dev as
 * nnet_backward takes it, and xent_grad_dev, the fp16 loss gradient [rows x P_xent] (leading
 * dimension P_xent) at the affine output of the log-softmax output layer named output-xent, as
 * kf_chain_xent writes it; both in the forward's row form (full rows, or the compact rows
 * under row subsampling). The xent branch (output-xent down to the branch point, a
 * linear-component on the chain output's path: prefinal-l) gets its weight gradients, and every
 * layer from the branch point down the gradient of both outputs: the branch's gradient at the
 * branch point is rounded to fp16 once (gx) and added in the input-gradient epilogue of the
 * chain-path layer above the branch point, g = rne(acc + gx). An error on a net without
 * output-xent, when the path from it does not reach the chain output's path, when the branch
 * point is not a linear-component, in MXFP8 mode and on a net bound to data parallel. With
 * natural gradient on, the branch's components keep plain gradients. nnet_backward is
 * unchanged: it zeroes the branch's gradients. */
int nnet_backward_xent(KfNet *net, const void *out_grad_dev, const void *xent_grad_dev);
float *nnet_grad_buffer(KfNet *net);   /* device fp32 [num_params] */
/* use caller-owned device memory (>= num_params fp32) as the gradient buffer */
int nnet_bind_grad_buffer(KfNet *net, float *dev);
float *nnet_master_buffer(KfNet *net); /* device fp32 [num_params] */
/* device fp16 [num_params]. A host that writes weights through this pointer (a
 * checkpoint restore, a weight broadcast) calls nnet_weights_changed afterwards, at
 * every such write: the forward of the TDNN-F affine and prefinal big layers reads
 * transposed copies and the fp8 mode MXFP8 copies, both derived from these weights. */
void *nnet_weight_buffer(KfNet *net);
/* the fp16 weights were written from outside: refresh the derived copies (transposed
 * copies at the next forward, MXFP8 copies now) */
int nnet_weights_changed(KfNet *net);
int nnet_sgd(KfNet *net, float lr, float momentum);

/* Kaldi-style parameter update (kf_ops.h kf_update_maxchange): momentum SGD
 * with a per-component max-change, L2 term and learning-rate factor, and a global limit on
 * the parameter change of one step.
 * The trainable tensors are grouped into components, one per Kaldi nnet3 component, under
 * the names nnet_load_kaldi reads: conv-relu-batchnorm <layer>.conv {W, Bias}; tdnnf
 * <layer>.linear {LinearW} and <layer>.affine {AffineW, AffineBias}; linear-component
 * <layer> {W}; prefinal prefinal-chain.affine | prefinal-xent.affine {BigW, BigBias} and
 * .linear {SmallW}; output and attention <layer>.affine {W, Bias}. A component's tensors are
 * consecutive: nnet_param_info(first_tensor .. first_tensor + num_tensors - 1); its segments
 * of the flat buffer are each tensor's rows * cols elements (the alignment padding between
 * tensors belongs to no component and is never touched).
 * Options come from the xconfig keys max-change (default 0.75, output layers 1.5; 0 = no
 * limit), l2-regularize (0) and learning-rate-factor (1) of the layer, which apply to both
 * components of a two-component layer; nnet_set_component_opts overrides them.
 * nnet_num_components, nnet_component_info and nnet_set_component_opts work on a
 * layout-only net. Any out pointer may be NULL. */
int nnet_num_components(const KfNet *net);
int nnet_component_info(const KfNet *net, int idx, char *name, int namelen, float *max_change, float *l2,
                        float *lr_factor, int *first_tensor, int *num_tensors);
/* max_change >= 0, l2 >= 0, lr_factor > 0; an unknown name or a bad value is an error */
int nnet_set_component_opts(KfNet *net, const char *name, float max_change, float l2, float lr_factor);
/* One update of the master / fp16 / velocity buffers from the gradient buffer (as nnet_sgd:
 * after nnet_backward, also a data-parallel one), asynchronous on the current stream.
 * max_param_change >= 0 (0 = no limit; Kaldi's default is 2.0); l2_scale is Kaldi's factor on
 * the L2 term, normally the minibatch's supervised frame count. The component tables and the
 * scratch are uploaded / allocated at the first call and again after
 * nnet_set_component_opts; nothing is allocated per step. Refreshes the derived weight
 * copies as nnet_sgd does. */
int nnet_update(KfNet *net, float lr, float momentum, float max_param_change, float l2_scale);
/* Kaldi's per-component max-change report of the last nnet_update (synchronises): the
 * step's norm n_c and scale s_c of components 0 .. n-1 (n <= nnet_num_components), the
 * global norm N and scale S. */
int nnet_update_stats(KfNet *net, float *norms, float *scales, int n, float *global_norm, float *global_scale);

/* Dynamic loss scaling of the fp16 train step, kept on the device (kf_ops.h kf_loss_scale_*,
 * DESIGN.md §30). The objective multiplies its derivative by the scale (hand
 * nnet_loss_scale_ptr to kf_chain.h kf_chain_set_grad_scale); nnet_backward is linear in its
 * seeds, so the gradient buffer then holds scale * G (after a data-parallel all-reduce: the
 * mean of the ranks' scaled gradients, an inf reaching every rank). While the mode is on, nnet_sgd
 * and nnet_update first check every trainable element of the gradient buffer (the update's
 * segment table; the alignment padding between tensors is not read) for a non-finite value and
 * advance the state, then run the update with the state: on an overflow the step is skipped
 * (master, fp16 weights and velocity keep their bits, the scale is multiplied by backoff, and a
 * skipped nnet_update reports all-zero stats), else the update reads g / scale. No host
 * synchronisation per step and no allocation after the set call.
 *   nnet_set_loss_scale        opts NULL: off, nnet_sgd / nnet_update are the plain calls. Else the
 *                              state is allocated (once per net) and initialised from opts. Refused
 *                              beside natural gradient (its Fisher state is not scale-equivariant
 *                              across a change of the scale) and MXFP8 mode (block scales of its own),
 *                              in either order.
 *   nnet_loss_scale_ptr        the device float holding the scale, NULL while off
 *   nnet_set_loss_scale_value  the scale (clamped to [min_scale, max_scale]), since = 0: a
 *                              checkpoint restore, tests
 *   nnet_loss_scale_stats      synchronises; any out pointer may be NULL. steps / skipped count the
 *                              updates since nnet_set_loss_scale, last_overflow is the last check's. */
int nnet_set_loss_scale(KfNet *net, const KfLossScaleOpts *opts);
const float *nnet_loss_scale_ptr(const KfNet *net);
int nnet_set_loss_scale_value(KfNet *net, float scale);
int nnet_loss_scale_stats(KfNet *net, float *scale, int *since, long long *steps, long long *skipped,
                          int *last_overflow);

/* Semi-orthogonal constraint (kf_ops.h kf_orthonormal_constrain): Kaldi's
 * ConstrainOrthonormal, which keeps a TDNN-F bottleneck matrix and the prefinal layers' small
 * projection close to semi-orthogonal. Every update component whose tensor is one weight
 * matrix W [K x n] carries a constraint value c: 0 off, > 0 a fixed scale, < 0 the floating
 * scale. It comes from the xconfig key orthonormal-constraint: default -1 on a tdnnf-layer
 * (its <layer>.linear, never .affine) and a prefinal-layer (its .linear, SmallW), 0 on a
 * linear-component; every other component is at 0. The first three entry points work on a
 * layout-only net. */
int nnet_component_orthonormal(const KfNet *net, int idx, float *c);
/* An unknown name, a component that is not a single weight matrix, a non-finite c, or a
 * c != 0 on a shape the kernel does not take (it needs K and n multiples of 32,
 * 32 <= n <= K, n <= 512; n > K is Kaldi's transposed case, not supported) is an error. */
int nnet_set_component_orthonormal(KfNet *net, const char *name, float c);
/* The constrained components (c != 0), in nnet_component_info order: returns their number
 * and writes the component indices of the first n to idx (may be NULL). */
int nnet_orthonormal_components(const KfNet *net, int *idx, int n);
/* One application of the constraint to every constrained component's fp32 master matrix and
 * its fp16 copy (the velocity is not touched), asynchronous on the current stream. Kaldi
 * skips each component at random with probability 3/4; here every constrained component is
 * handled at every call and the schedule is the caller's (every fourth step gives Kaldi's
 * rate). The matrix table and the scratch are uploaded / allocated at the first call and again
 * after nnet_set_component_orthonormal; nothing is allocated per call. Refreshes the derived
 * weight copies as nnet_sgd does. A net without a constrained component returns 0 and
 * launches nothing. */
int nnet_constrain_orthonormal(KfNet *net);
/* The report of the last nnet_constrain_orthonormal (synchronises), measured before that
 * call's update: scale s, ratio (1 with a fixed scale) and err = |W^T W - s^2 I|_F of the
 * first n constrained components (n <= nnet_orthonormal_components; s = 0: the matrix was
 * all-zero or not finite and was left untouched). Any out pointer may be NULL. */
int nnet_orthonormal_stats(KfNet *net, float *scale, float *ratio, float *err, int n);

/* Natural-gradient preconditioning of the weight gradients (kf_ops.h kf_ng_*):
 * Kaldi's NG-SGD, the online natural-gradient method of Povey, Zhang and Khudanpur. With the
 * switch on, nnet_backward leaves in the gradient buffer, for every preconditioned component,
 *   G^ = gamma_in gamma_out (I - W_in^T W_in) G (I - W_out^T W_out)
 * instead of the plain G = X_ext^T dY (X_ext: the layer input as the weight gradient sees it, with
 * the time splice and, for a component with a bias, an appended column of ones, so that G stacks
 * dW over db), and advances the two preconditioners' states; nnet_sgd and nnet_update then see
 * G^ with no change to either. Preconditioned: the update components of linear, output,
 * tdnnf (.linear and .affine) and prefinal (.affine, .linear) layers on the output's path; conv,
 * attention and per-sequence components keep plain gradients. opts: kf_ng_default_opts gives
 * Kaldi's values (rank_in 20, rank_out 80, update_period 4, num_samples_history 2000, alpha 4).
 * A side's rank is clamped to half its dimension (and to KF_NG_MAX_RANK); a side whose rank
 * would be below 8 is left unpreconditioned. NULL turns the switch off: nnet_backward is then
 * what it was, bit for bit. Setting it (again) allocates the state and scratch and starts every
 * preconditioner from the default initial state; nothing is allocated per step. An error in
 * MXFP8 mode, on a net bound to data parallel (and nnet_set_fp8 / nnet_bind_dp fail while it
 * is on), with implicit dz, and in nnet_backward_n. */
int nnet_set_natural_gradient(KfNet *net, const KfNgOpts *opts);
/* the preconditioners (one per preconditioned side of a component), 0 when off */
int nnet_natural_gradient_count(const KfNet *net);
/* The report of the last nnet_backward (synchronises) for preconditioners 0 .. n-1: the update
 * component (nnet_component_info index), the side (0 in, 1 out) and KF_NG_REPORT floats each:
 * gamma, rho, sum(d), t (all before that step's state update), and a flag that is 1 when a
 * non-finite statistic, eigenvalue or result made the update leave the state untouched. Any out
 * pointer may be NULL. */
int nnet_natural_gradient_stats(KfNet *net, int *component, int *side, float *report, int n);
/* State read-back of preconditioner idx (synchronises), for tests and checkpoints: W [rank x dim]
 * fp32, d [rank], rho, t. Any out pointer may be NULL (query dim and rank first). */
int nnet_natural_gradient_state(KfNet *net, int idx, int *component, int *side, int *dim, int *rank, float *W,
                                double *d, double *rho, double *t);

/* Per-sequence dropout of the TDNN-F layers (kf_ops.h kf_dropout_masks): Kaldi's
 * tdnnf-layer is linear -> affine -> ReLU -> BatchNorm -> dropout -> + bypass-scale * input,
 * the dropout a GeneralDropoutComponent with continuous=true, time-period=0, block-dim=dim: one
 * factor m = (1 - 2p) + 4p u, u ~ U[0, 1), per (sequence, column), shared by all frames of the
 * sequence, mean 1, no rescaling; the bypass does not go through it. A tdnnf-layer has the
 * component when its xconfig line carries dropout-proportion >= 0 (the key's default, -1,
 * means none; allowed: -1 or [0, 0.5]). With the switch on, the affine GEMM's epilogue applies
 *   y = rne((relu(z) scale + shift) m[b][n] + bypass x)
 * and the input-gradient GEMM that produces the layer's dz writes
 *   dz = rne(v bnscale[n] m[b][n] relu_bit)
 * so weight gradients, bottleneck gradients and NG-SGD need no change. Every call below but
 * nnet_dropout_mask works on a layout-only net.
 *
 * nnet_set_sequences: the sequence boundaries of later nnet_forward calls with
 * T == seq_row0[B] (seq_row0 host int[B + 1], seq_row0[0] = 0, strictly increasing, as
 * nnet_forward_ivector's, which sets them itself); NULL, 0 or no call: the whole input is one
 * sequence. With dropout on, a forward whose T differs from the boundaries given fails. */
int nnet_set_sequences(KfNet *net, const int *seq_row0, int B);
/* the layers with a dropout component (nnet_layer_info indices): returns their number and
 * writes the first n to idx (may be NULL) */
int nnet_dropout_layers(const KfNet *net, int *idx, int n);
/* Kaldi's set-dropout-proportion: 0 <= p <= 0.5 on the named layer, or with layer = NULL on
 * every layer with a component. A named layer without a component is an error. */
int nnet_set_dropout_proportion(KfNet *net, const char *layer, float p);
/* a layer's current proportion, -1 when it has no component */
int nnet_dropout_proportion(const KfNet *net, const char *layer, float *p);
/* The switch (default off: test mode) and the generator's 64-bit seed. Off, or every
 * proportion 0, leaves forward and backward what they were, bit for bit. While on, each
 * forward draws the masks of (seed, step) for every layer with p > 0 (one launch) and the step
 * then advances by one, masks drawn or not; the backward uses the masks of its forward. The
 * mask tables grow with the largest number of sequences seen; nothing is allocated per step.
 * On a net with a dropout component: an error in MXFP8 mode and with implicit dz, and while
 * on, nnet_set_fp8, nnet_set_implicit_dz and nnet_backward_n fail. The step is not reset. */
int nnet_set_dropout(KfNet *net, int on, unsigned long long seed);
/* the step the next forward draws with (0 <= step < 2^32; it wraps there): replay */
int nnet_set_dropout_step(KfNet *net, long long step);
long long nnet_dropout_step(const KfNet *net);
/* the mask the last forward drew for a layer (synchronises): host fp32 [B x dim] (NULL: only
 * B and dim). An error when that forward drew none for it (dropout off, p = 0). */
int nnet_dropout_mask(KfNet *net, const char *layer, float *host, int *B, int *dim);

/* SpecAugment of the spec-augment-layer (kf_ops.h kf_specaug_rows): Kaldi's
 * frequency mask (one zeroed band of at most Z = min(D, floor(D f + 0.5)) columns per sequence)
 * and time mask (alternating kept and zeroed runs of frames, zeroed ones at most m frames long,
 * about the share z of all frames) on the layer's input; zeroed elements are +0, nothing is
 * rescaled. The layer reads the xconfig keys freq-max-proportion f in [0, 1] (default 0.5),
 * time-zeroed-proportion z in [0, 1) (default 0.2) and time-mask-max-frames m >= 1 (default 10).
 * Every call below but nnet_spec_augment_rows works on a layout-only net.
 *
 * nnet_spec_augment_layers: the spec-augment layers (nnet_layer_info indices) in the order of
 * their ordinals: returns their number and writes the first n to idx (may be NULL). */
int nnet_spec_augment_layers(const KfNet *net, int *idx, int n);
/* a named spec-augment layer's options (each pointer may be NULL), and setting them, with the
 * ranges of the xconfig keys */
int nnet_spec_augment_opts(const KfNet *net, const char *layer, double *f, double *z, int *m);
int nnet_set_spec_augment_opts(KfNet *net, const char *layer, double f, double z, int m);
/* The switch (default off: test mode, the identity) and the generator's 64-bit seed. A layer is
 * active in a forward when the switch is on and (Z > 0 or z > 0). An active layer has an
 * activation of its own, fp16 [max_frames x dim] (allocated at the first forward that needs it,
 * never per step), written by two launches (kf_specaug_rows, kf_specaug_apply) from the masks
 * of (seed, step, the layer's ordinal); its consumers, nnet_activation and the backward (the
 * weight gradient of the conv above) read that masked activation. An inactive layer stays an
 * alias of its input: forward and backward are what they were, bit for bit. Sequences are those
 * of nnet_set_sequences / nnet_forward_ivector; with the switch on, a forward whose T differs
 * from the boundaries given fails. The feature's own step counter advances at every forward
 * while the switch is on (on a net with such a layer) and wraps at 2^32. Switching on while a
 * consumer of a spec-augment layer would read an MXFP8 copy of the layer's input
 * (nnet_set_fp8) is an error, as is nnet_set_fp8 then. Backward through the layer into a
 * trainable layer below it is not supported (Kaldi's recipes have none). */
int nnet_set_spec_augment(KfNet *net, int on, unsigned long long seed);
/* the step the next forward draws with (0 <= step < 2^32): replay */
int nnet_set_spec_augment_step(KfNet *net, long long step);
long long nnet_spec_augment_step(const KfNet *net);
/* the row_band (kf_ops.h kf_specaug_rows) the last forward drew for a layer (synchronises):
 * host int32 [T] (NULL: only T). An error when that forward drew none for it. */
int nnet_spec_augment_rows(KfNet *net, const char *layer, int32_t *host, int *T);

/* Training-mode BatchNorm (default off): Kaldi's BatchNormComponent in
 * training mode for the BatchNorms the switch governs (nnet_bn_train_layers: their layer indices
 * in layer order, a prefinal layer once; returns their number). Which kinds of layer those are is
 * nnet_set_bn_train_sites' mask of
 *   KF_BN_SITE_TDNNF      BatchNorm 0 of every tdnnf-layer (the default, alone),
 *   KF_BN_SITE_CONV       every conv-relu-batchnorm-layer: block-dim = num-filters-out, the
 *                         statistics of a filter run over rows x height-out,
 *   KF_BN_SITE_PREFINAL   both BatchNorms of every prefinal-layer (0: big-dim, behind the ReLU;
 *                         1: small-dim, no ReLU), prefinal-xent included,
 *   KF_BN_SITE_COMPONENT  every batchnorm-component (a per-sequence one, ivector-batchnorm, over
 *                         its B rows),
 * KF_BN_SITE_ALL for Kaldi's behaviour; nnet_bn_train_sites reads it. The setter is refused while
 * the switch is on and governs a layer (set while it governed none, the switch goes on for the new
 * sites). The attention layer's BatchNorm is fused into its kernel and stays frozen.
 * While the switch is on, each nnet_forward normalises a governed BatchNorm by the statistics of
 * its own rows (all rows the layer computes, every frame once; kf_ops.h kf_bn_train_stats,
 * kf_bn_block_stats), nnet_backward differentiates through them, and the BatchNorm accumulates
 * count, sum and sumsq in double. The frozen statistics (nnet_set_bn) are untouched and apply
 * again when the switch is off. Storage for a site (its r tensor: a conv layer's is as large as
 * its activation) is made the first time the switch goes on with the site selected.
 *   nnet_bn_dim: the length of a BatchNorm's statistics: num-filters-out for conv, big-dim /
 *     small-dim for prefinal `which` 0 / 1, out_dim otherwise; -1 when the layer has none.
 *   nnet_bn_batch_stats: mean / var [nnet_bn_dim] of the last forward (fp32; either may be NULL).
 *   nnet_bn_stats: the accumulators (count; sum, sumsq [nnet_bn_dim]; any may be NULL).
 *   nnet_bn_zero_stats: clears them (Kaldi's ZeroComponentStats at the start of a job).
 *   nnet_bn_commit: every governed BatchNorm with count > 0 takes mean = sum / count,
 *     var = sumsq / count - mean^2 (floored at 0) as its frozen statistics through nnet_set_bn
 *     (gamma 1, beta 0, its own eps and target_rms); returns the layers committed, -1 on error.
 * `which` is the BatchNorm index of nnet_set_bn (1: prefinal-layer's second one). Composes with
 * dropout, SpecAugment, natural gradient, nnet_update, the orthonormal constraint and
 * nnet_backward_xent. Refused, in either order of the two calls: MXFP8 mode (nnet_set_fp8),
 * implicit dz, row subsampling under the default row policy (the compact row set's scratch row
 * and inexact tail rows are not rows of the layer), a bound data-parallel communicator (the
 * statistics would be each rank's own), and nnet_backward_n. With KF_BN_SITE_COMPONENT, a
 * frame-level batchnorm-component above a trainable layer is refused by nnet_set_bn_train (none of
 * the recipes has one).
 *
 * nnet_set_bn_train_rows (default KF_BN_ROWS_ALL, the rule above):
 * KF_BN_ROWS_SUBSAMPLED lets the switch and nnet_set_row_subsampling(3) be on together, in either
 * order. In a forward that ran on the compact rows (nnet_row_set: tc > 0), a governed BatchNorm of
 * a compact layer (tdnnf-layers, both BatchNorms of a prefinal-layer, prefinal-xent included) takes
 * mean and var from the rows c < tc0, the source rows 0 (mod 3), which are exact at every layer;
 * all tc rows are normalised by them and count grows by tc0. The backward is that forward's exact
 * derivative: a, b summed over all tc rows and divided by tc0, the correction on the rows c < tc0
 * only (kf_ops.h kf_bn_train_bwd_stats_rows / _apply_rows). A forward on full rows (row
 * subsampling off, fp8, a short T) keeps the all-rows rule, and so does every layer below the row
 * set. A conv-relu-batchnorm-layer directly below the row set that the switch governs
 * (KF_BN_SITE_CONV) runs on full rows and is gathered, as with KF_RSUB_CONV=0. The policy cannot be
 * changed while both modes are on; it needs no device (works on a layout-only net).
 * nnet_bn_train_rows reads it. */
#define KF_BN_SITE_TDNNF 1
#define KF_BN_SITE_CONV 2
#define KF_BN_SITE_PREFINAL 4
#define KF_BN_SITE_COMPONENT 8
#define KF_BN_SITE_ALL 15
int nnet_set_bn_train(KfNet *net, int on);
int nnet_set_bn_train_sites(KfNet *net, int sites);
int nnet_bn_train_sites(const KfNet *net);
int nnet_bn_train_layers(const KfNet *net, int *idx, int n);
#define KF_BN_ROWS_ALL 0
#define KF_BN_ROWS_SUBSAMPLED 1
int nnet_set_bn_train_rows(KfNet *net, int policy);
int nnet_bn_train_rows(const KfNet *net);
int nnet_bn_dim(const KfNet *net, const char *layer, int which);
int nnet_bn_batch_stats(KfNet *net, const char *layer, int which, float *mean, float *var);
int nnet_bn_stats(KfNet *net, const char *layer, int which, double *count, double *sum, double *sumsq);
int nnet_bn_zero_stats(KfNet *net);
int nnet_bn_commit(KfNet *net);

/* ReLU unit statistics and self-repair: Kaldi's StoreStats and
 * RectifiedLinearComponent::RepairGradients on the train step. A site is a ReLU that training-mode
 * BatchNorm governs: a tdnnf-layer, the big affine of a prefinal-layer or a conv-relu-batchnorm
 * layer in the current nnet_set_bn_train_sites set with nnet_set_bn_train on; its D columns are
 * nnet_bn_dim(layer, 0). While the switch is on, every forward in the mode adds, per site, over the
 * rows its BatchNorm statistics run over: count += n, deriv_sum[c] += #{rows : r > 0} (device
 * doubles, exact), from the statistics pass that reads r anyway. Every backward first builds each
 * site's repair vector in one launch: s[c] = -scale S where deriv_sum[c] <= lower count (a dead
 * unit), +scale S where deriv_sum[c] > upper count (a saturated one), else 0 (and 0 while count
 * is 0); S is the loss scale's device value, 1 with the loss scale off. The site's
 * dz = rne_fp16(scale (dy - a - yhat b) relu_bit + s) on the statistics rows: after one nnet_sgd
 * step with a positive learning rate a dead unit's bias is larger than before. Every step, at the
 * plain scale (Kaldi: a random half of the minibatches, at twice the scale).
 *   nnet_set_self_repair: the switch. Where no site exists (training-mode BatchNorm off, or no such
 *     layer in its sites) it is accepted and no pass changes. Refused beside MXFP8, implicit dz,
 *     data parallel and nnet_backward_n, in either order. For those refusals the switch counts from
 *     the moment it is set on a net whose nnet_set_bn_train_sites hold a layer with a ReLU, whether
 *     training-mode BatchNorm is on or not: while it is set, nnet_set_fp8, nnet_set_implicit_dz,
 *     nnet_bind_dp and nnet_backward_n fail even though no site is active yet.
 *   nnet_self_repair_sites: the layer indices of the sites while the mode is on (as nnet_bn_train_layers).
 *   nnet_self_repair_opts / nnet_set_self_repair_opts: a layer's scale, lower and upper threshold
 *     (xconfig self-repair-scale, self-repair-lower-threshold, self-repair-upper-threshold; 1e-5,
 *     0.05, 0.95); scale >= 0 and 0 <= lower < upper <= 1, else -1. Need no device.
 *   nnet_relu_stats: synchronises. count, and [D] each: value_sum (the BatchNorm accumulator's sum)
 *     and deriv_sum; value_sum / count and deriv_sum / count are Kaldi's <ValueAvg> and <DerivAvg>
 *     as long as both kinds were cleared together. Any pointer may be NULL.
 *   nnet_relu_zero_stats: clears the ReLU statistics and the BatchNorm accumulators
 *     (nnet_bn_zero_stats): Kaldi's ZeroComponentStats clears both kinds.
 *   nnet_self_repair_vector: the last backward's s [D] of a site (fp32), for tests and diagnostics. */
int nnet_set_self_repair(KfNet *net, int on);
int nnet_self_repair_sites(const KfNet *net, int *idx, int n);
int nnet_self_repair_opts(const KfNet *net, const char *layer, float *scale, double *lower, double *upper);
int nnet_set_self_repair_opts(KfNet *net, const char *layer, float scale, double lower, double upper);
int nnet_relu_stats(KfNet *net, const char *layer, double *count, double *value_sum, double *deriv_sum);
int nnet_relu_zero_stats(KfNet *net);
int nnet_self_repair_vector(KfNet *net, const char *layer, float *host);

/* MXFP8 train step (BASELINE configs[4]): 1 = every TDNN-F / linear / prefinal / output
 * GEMM whose input has an MXFP8 copy runs on the fp8 MFMA (kf_ops.h MXFP8 operands);
 * the producing epilogues write those copies, weights are re-quantised on every
 * parameter change; in the backward the strided TDNN-F affine input gradients run on
 * e4m3 copies of dz (written by the layer above's input-gradient epilogue) and of W2,
 * everything else stays fp16. 2 = the same forward with an all-fp16 backward (a test
 * knob). 0 = off. */
int nnet_set_fp8(KfNet *net, int on);

/* Data parallel (kf_dp.h). nnet_bind_dp: nnet_backward exchanges the
 * gradient in buckets of >= bucket_bytes, each all-reduced (average over ranks) on
 * the communicator's stream as soon as the backward has enqueued the weight-gradient
 * kernels of every parameter in it, in reverse layer order; it returns with the
 * compute stream waiting for the last bucket. dp = NULL unbinds.
 * nnet_dp_plan: that bucket plan (kf_dp_plan's outputs; works on a layout-only net). */
typedef struct KfDp KfDp;
int nnet_bind_dp(KfNet *net, KfDp *dp, long long bucket_bytes);
int nnet_dp_plan(const KfNet *net, long long bucket_bytes, int max_buckets, int *after_step,
                 long long *begin, long long *end);
/* nnet_bind_dp plans at most 256 buckets (the rest merges into the final one).
 * Test hook: on != 0 issues every bucket at the start of nnet_backward, before any
 * gradient exists: the negative control of the overlap tests (kf_dp_debug). */
int nnet_dp_debug_early(KfNet *net, int on);

/* Weight gradients on a second stream (default on): nnet_backward launches every dW / db
 * GEMM (and the data-parallel bucket gates) on a stream of its own, ordered by events after
 * the producers on the caller's stream, so they overlap the input-gradient chain; the
 * caller's stream waits for them before nnet_backward returns. 0 = everything on the
 * caller's stream (the r4 order, A/B and tests). */
int nnet_set_wgrad_stream(KfNet *net, int on);

/* Row-subsampled train step (r6; default off). stride = 3 declares that the caller reads the
 * output, and writes output gradients, on rows 0 (mod 3) only (the chain objective with
 * frame-subsampling-factor 3 and every eg's first supervised row at 0 mod 3, as
 * chain_layout / TrainStep lay them out). The layers at the top of the output chain whose
 * row t depends only on rows t and t +- 3 of the layer below (TDNN-F with time stride 0 or
 * 3, linear, prefinal, output, above a conv-relu-batchnorm layer) then run on the rows
 * those outputs depend on — Kaldi nnet3's computation of only the indexes an output needs:
 * the rows 0 (mod 3) and, through the splices' clamp at T - 1, a tail of rows
 * T-1, T-4, ... — so each of those layers' forward and backward does a third of the work.
 * Output rows of the set, the objective, every weight gradient and the gradient into the
 * conv stack are those of the full computation (weight gradients up to the split-K
 * summation order). After nnet_forward, nnet_row_set gives the compact rows tc (0 = this
 * forward ran on full rows: fp8, implicit dz or a short T) and tc0: compact row c holds
 * source row 3c for c < tc0, else (T-1) - 3(tc-1-c); those layers' activations
 * (nnet_activation: rows = tc) and the output gradient nnet_backward reads are in compact
 * rows. stride 0 / 1: off. */
int nnet_set_row_subsampling(KfNet *net, int stride);
int nnet_row_set(const KfNet *net, int *tc, int *tc0);

/* Implicit dz (default off; fp16 steps): the input-gradient GEMM that produces a TDNN-F
 * layer's output gradient g (layers with a bypass, which store g anyway) does not also
 * store dz = rne(g * bnscale * relu_mask). The layer's affine weight gradient and input
 * gradient read g through the forward's ReLU mask (masked operands, kf_ops.h); the BN scale
 * multiplies the weight gradient's columns in its split-K reduction and is folded into a
 * scaled fp16 copy of W2 for the input gradient. Rounding points change accordingly (the
 * oracle's OrcNet.implicit_dz follows them). Measured step-neutral, hence
 * off: 0 = store dz (the default). */
int nnet_set_implicit_dz(KfNet *net, int on);

/* diagnostics (tests) of the two-stream backward: main_aff chooses where the TDNN-F
 * affine weight gradients run (0, the default, and -1: all on the
 * weight-gradient stream; 1 = every other one on the input-gradient chain; 2 = all on the
 * chain);
 * stall_cycles > 0 queues a spin kernel of that many GPU clock cycles (kf_debug_spin) on
 * the weight-gradient stream before each of its batches of work, so that stream runs far
 * behind the chain and any missing order shows as a wrong gradient. */
int nnet_debug_backward(KfNet *net, int main_aff, long long stall_cycles);

/* diagnostics (tests): the device blocks the net holds at this moment (-1: null net). A switch
 * allocates what it needs when it is first set; setting it again does not grow the count. */
int nnet_debug_alloc_count(const KfNet *net);

/* diagnostics (tests): back-propagate through the top n layers only; device
 * pointer of an internal tensor ("dz0" .. "dz2", "g0" .. "g2": the backward's gradient ring,
 * "dzlast": the ring buffer the last step wrote, "dbott" (the buffer of the last
 * TDNN-F / prefinal step), "aux", "mask",
 * "bn_scale", "bn2_scale", "dproj" (attention: the gradient of its affine output), "gdb" (a
 * combine-feature-maps layer: the per-sequence gradient [B x height * num-filters2] of its second
 * input), and with fp8 on "x8q" / "x8s": the e4m3 values
 * [T x pad128(in_dim)] and E8M0 scales [T x pad128(in_dim)/32] of the MXFP8 input copy
 * the layer's GEMM reads; "w8dq" / "w8ds": a strided TDNN-F layer's e4m3 affine weight rows
 * for its MXFP8 input gradient [bottleneck x 2*pad128(out_dim)]; "dz8q" / "dz8s" with
 * layer = 0 .. 2: the e4m3 copy of dz0 .. dz2, and "dz8layer": 1 + the layer that copy is
 * for, as the returned pointer value (NULL: none); `layer` selects the per-layer ones),
 * NULL if unknown */
int nnet_backward_n(KfNet *net, const void *out_grad_dev, int n);
const void *nnet_debug_tensor(KfNet *net, const char *what, int layer);

#ifdef __cplusplus
}
#endif
#endif
