// loss_scale_state.h — the device state block of the dynamic loss scale (kf_ops.h
// kf_loss_scale_*), read by the update kernels (update.hip, layers.hip) and written
// by loss_scale.hip.
#pragma once

// scale first: it is what the objective's kernels read through kf_chain_set_grad_scale. Written
// by one lane of k_ls_advance (and by the one-thread k_ls_init / k_ls_set), read block-uniformly
// by the update kernels.
struct KfLossScaleState {
    float scale;     // the next objective's factor
    float inv_used;  // 1 / the scale the gradient under check was made with (latched by the advance)
    int since;       // clean steps since the last change of the scale
    int skip;        // the last check found a non-finite element: the update kernels return at once
    long long steps, skipped;
    int last_overflow;  // = skip, kept for the report
    int growth_interval;
    float growth, backoff, min_scale, max_scale;
};
