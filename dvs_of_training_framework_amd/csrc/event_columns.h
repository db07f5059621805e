// The two forms in which the per-event columns reach the events-only terms
// (contrast.hip, avg_timestamp.hip): the wire columns of the reference's
// collate (x, y, polarity, sample_index as int64, timestamp as float32, 36
// bytes an event) and the encoded columns of a preprocessed dataset as stored
// (int16 x, int16 y, float32 timestamp, bool polarity, 9 bytes an event, with
// the first event of every sample: include/dvsof_event_terms_encoded.h).  An
// event kernel takes its loader as a template parameter by value, reads an
// event once at the top of its loop and shares everything below the load, so
// both forms give the same bytes: all sums are integer atomics.
#pragma once
#include "event_images.h"

namespace {

// one event as every kernel sees it
struct EventRow {
    int64_t x, y;
    float t;
    int64_t sample;
    int sign;  // of the polarity: -1, 0 or +1; 0 where the call has no polarity channels
};

// the reference's wire format
struct WireColumns {
    const int64_t *x, *y;
    const float *t;
    const int64_t *pol, *sample;  // pol may be null without polarity channels: it is not read then

    bool given(int polarity) const { return x && y && t && sample && (!polarity || pol); }

    template <bool POL>
    __device__ __forceinline__ EventRow load(int64_t e) const
    {
        int sign = 0;
        if (POL) {
            const int64_t pe = pol[e];
            sign = pe > 0 ? 1 : (pe < 0 ? -1 : 0);
        }
        return EventRow{x[e], y[e], t[e], sample[e], sign};
    }
};

// the encoded columns + the first event of every sample.  The sample of event
// e is the largest b in [0, B) with ev_off[b] <= e (the rule of
// dvsof_voxelize_encoded and of learned_voxel.hip): empty samples are repeated
// offsets, and a slot at or past ev_off[B] falls to sample B - 1.
struct EncodedColumns {
    const int16_t *x, *y;
    const float *t;
    const uint8_t *pol;     // may be null without polarity channels
    const int64_t *ev_off;  // [B + 1]
    int B;

    bool given(int polarity) const { return x && y && t && ev_off && B >= 1 && (!polarity || pol); }

    template <bool POL>
    __device__ __forceinline__ EventRow load(int64_t e) const
    {
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (ev_off[mid] <= e) lo = mid; else hi = mid;
        }
        int sign = 0;
        if (POL) sign = pol[e] ? 1 : -1;
        return EventRow{(int64_t)x[e], (int64_t)y[e], t[e], (int64_t)lo, sign};
    }
};

// The channel of an event from the sign its loader gave: 0 without polarity,
// else 0 for +1 and 1 for -1; false: sign 0, in neither channel and in no count.
// The two terms state the rule here, once for both column forms (the overload
// of event_images.h that reads a polarity column itself is iwe.hip's).
template <bool POL>
__device__ __forceinline__ bool event_channel(int sign, int &c)
{
    c = 0;
    if (POL) {
        if (sign == 0) return false;
        c = sign < 0;
    }
    return true;
}

}  // namespace
