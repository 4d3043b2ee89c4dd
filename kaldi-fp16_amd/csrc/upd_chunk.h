// upd_chunk.h — how the kernels over a kf_update_maxchange segment table (kf_ops.h) cut it into
// workgroups, shared by update.hip and loss_scale.hip (the dynamic loss scale's check pass,
// DESIGN §30).
#pragma once
#include "kf_common.h"
#include "../../include/kf_ops.h"
#include "loss_scale_state.h"

namespace {

// the chunk of workgroup b: elements [cb, ce) of component comp; false when b is past the table
__device__ __forceinline__ bool upd_chunk(const KfUpdSegment *segs, int nseg, int ncomp, long long n, int b,
                                          long long &cb, long long &ce, int &comp) {
    int lo = 0, hi = nseg;  // the first segment whose first_wg lies above b
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].first_wg > b) hi = mid;
        else lo = mid + 1;
    }
    if (lo == 0) return false;
    const KfUpdSegment s = segs[lo - 1];
    // a table that does not fit the buffer addresses nothing outside [0, n)
    const long long sb = s.begin < 0 ? 0 : s.begin, se = s.end > n ? n : s.end;
    cb = sb + (long long)(b - s.first_wg) * KF_UPD_CHUNK;
    if (cb >= se) return false;
    ce = cb + KF_UPD_CHUNK < se ? cb + KF_UPD_CHUNK : se;
    comp = s.comp;
    return comp >= 0 && comp < ncomp;
}

// [cb, ce) = scalar head [cb, a0), float4 body [a0, a1), scalar tail [a1, ce); a0 % 4 == 0
__device__ __forceinline__ void upd_split(long long cb, long long ce, long long &a0, long long &a1) {
    a0 = (cb + 3) & ~3ll;
    if (a0 > ce) a0 = ce;
    a1 = a0 + ((ce - a0) & ~3ll);
}
// the (at most six) scalar elements of a chunk, one per thread: index or -1
__device__ __forceinline__ long long upd_scalar(long long cb, long long ce, long long a0, long long a1, int t) {
    const long long nh = a0 - cb;
    if (t < nh) return cb + t;
    const long long i = a1 + (t - nh);
    return i < ce ? i : -1;
}

// workgroups launched: at least one per chunk of any segment table over [0, n)
inline long long upd_grid(long long n, int nseg) { return n / KF_UPD_CHUNK + nseg; }

}  // namespace
