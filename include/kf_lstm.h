/*
 * kf_lstm.h — Kaldi's projected LSTM (fast-lstmp-layer) as a sequence operator on the MI355X:
 * forward and exact backward over B sequences concatenated row-wise. The network
 * layer (xconfig fast-lstmp-layer, parameter tables, row-set policy, mode table) is not built:
 * nnet_create still answers "type not supported" for it.
 *
 * Sizes: input width D, cell dim C, recurrent projection R, non-recurrent projection N, delay
 * d < 0. Sequence i owns rows [seq_row0[i], seq_row0[i+1]) of x and y. Per frame t of a sequence,
 * with r' = r[t+d] and c' = c[t+d] (zeros while t + d < 0, Kaldi's IfDefined):
 *   a   = W_x x_t + W_r r' + b                   gate blocks i, f, g, o of C columns each
 *   i   = sigmoid(a_i + w_ic * c')    f = sigmoid(a_f + w_fc * c')    g = tanh(a_g)
 *   c_t = f * c' + i * g
 *   o   = sigmoid(a_o + w_oc * c_t)   m_t = o * tanh(c_t)
 *   y_t = W_p m_t + b_p               r_t = y_t[0:R]      (the layer's output is y_t, width R + N)
 * x, y, m, the gate activations, G = X W_x + b and the working copy of every parameter are fp16;
 * c is fp32; a step's arithmetic is fp32 on the fp32 MFMA accumulators.
 *
 * Parameters (kf_lstmp_set_params / _get_params, and the gradient buffer of kf_lstmp_backward): one
 * flat fp32 array of kf_lstmp_num_params() values, every affine as nnet_grad_buffer lays one out
 * (weights [in x out] row-major, then the bias):
 *   W_x [D x 4C], b [4C], W_r [R x 4C], w_ic [C], w_fc [C], w_oc [C], W_p [C x (R+N)], b_p [R+N]
 *
 * Backward: the exact derivative of the forward, with the row-norm clip of Kaldi's
 * BackpropTruncationComponent on the derivative that flows back through r and through c at every
 * recurrence: a row (R values of dr, respectively C values of dc, of one frame) whose L2 norm
 * exceeds the threshold is scaled down to it. Threshold 30 by default, 0 = off. Kaldi's periodic
 * zeroing (zeroing-interval / zeroing-threshold) is not built.
 *
 * All work is asynchronous on kf_get_stream(); a call allocates nothing and replays bit for bit.
 * Returns: int 0 / -1 (NULL for the constructor) and kf_lstmp_last_error().
 */
#ifndef KF_LSTM_H
#define KF_LSTM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct KfLstmp KfLstmp;

/* kf_prof record classes (kf_ops.h kf_prof_collect) of one whole forward / backward call */
#define KF_PROF_LSTMP_FWD 8
#define KF_PROF_LSTMP_BWD 9

/* Workspace for calls of up to max_rows rows in up to max_seqs sequences. Refused, with a message
 * that names the rule: C, R or N not a multiple of 32 (N may be 0), R = 0, delay >= 0, D not a
 * multiple of 8, max_rows or max_seqs < 1. */
KfLstmp *kf_lstmp_create(int D, int C, int R, int N, int delay, int max_rows, int max_seqs);
void kf_lstmp_free(KfLstmp *l);
long long kf_lstmp_num_params(const KfLstmp *l);

/* The fp32 master (host array, layout above) and from it the fp16 working copies the kernels read,
 * rounded to nearest even. Synchronous. */
int kf_lstmp_set_params(KfLstmp *l, const float *params);
int kf_lstmp_get_params(const KfLstmp *l, float *params);

/* Row-norm clip threshold of the backward (>= 0; 0 = off; 30 after create). */
int kf_lstmp_set_clip(KfLstmp *l, float threshold);

/* y[rows x (R+N)] (fp16, leading dimension ldy) from x[rows x D] (fp16, leading dimension ldx, a
 * multiple of 8; x 16-byte aligned). seq_row0: host int32[B+1], non-decreasing from 0;
 * rows = seq_row0[B]. x must stay as it is until the backward of this forward has run. Refused:
 * rows beyond max_rows, sequences beyond max_seqs. */
int kf_lstmp_forward(KfLstmp *l, const void *x_dev, long long ldx, const int32_t *seq_row0, int B,
                     void *y_dev, long long ldy);

/* The backward of the last forward: dx[rows x D] (fp16, ldx a multiple of 8; NULL: not wanted)
 * from dy[rows x (R+N)] (fp16), and every parameter's gradient ADDED into grad_dev (fp32 device
 * array, layout above). */
int kf_lstmp_backward(KfLstmp *l, const void *dy_dev, long long ldy, void *dx_dev, long long ldx,
                      float *grad_dev);

/* Device pointers to what the last forward stored (tests): c fp32 [rows x C], m fp16 [rows x C],
 * gates fp16 [rows x 4C] (the activations i, f, g, o). Any out pointer may be NULL. */
int kf_lstmp_state(const KfLstmp *l, const float **c, const void **m, const void **gates);

const char *kf_lstmp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
