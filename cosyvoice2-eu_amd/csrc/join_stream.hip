// Continuous calls (an extension of the reference): the 24 kHz chunks of one call's text segments, as the streaming
// path produces them, written into ONE stream -- interior silences optionally gated away, a pause of zeros between the pieces, a short
// raised-cosine fade at each gated edge -- ahead of the output stage, chunk by chunk.  The per-segment trim of join.hip needs the
// segment's peak, which is known at its end only; the gate here is causal and its result does not depend on the chunk boundaries.
//
//   gate (cv2_wave_gate_chunk): frames of 240 samples, peak_f = max |s[q]| over the frame (NaN counts as 0); R(f) = max(C, peak_0 .. peak_f)
//     with C the maximum over every earlier segment; frame f is loud iff R(f) > 0 and peak_f >= R(f) * g (ONE fp32 product).  One block:
//     its four waves take the peaks of up to 256 frames into LDS, one wave scans them (running maximum, loud flags, first / last loud).
//     The samples of a frame come from the call's held buffer, from the new chunk, or from both.
//   emit (cv2_wave_emit_chunk): every output sample is a copy (bit for bit), a copy times one fade weight (one fp32 multiply), or +0.0f;
//     what stays held is compacted into the call's other buffer by the same launch.
//
// Per-call state on the device: cv2_wave_state (running-peak bits, C, frame phase, first / last loud frame, held count and position) and
// the held samples.  The host mirrors the integers (cv2amd/join.py: StreamPlan); the entry points check every range before they launch.
#include <limits.h>
#include "common.h"
#include "../../include/cv2_amd.h"

constexpr int GATE_FRAME = 240;                         // samples per frame (10 ms at 24 kHz), no overlap: WAVE_FRAME of join.hip
constexpr int GATE_TILE = 256;                          // frames per scan: 64 lanes x 4 consecutive frames
constexpr int EMIT_TO = 1024;                           // outputs per block: 256 threads x 4 consecutive outputs
constexpr int MAX_FADE = 120;                           // F <= 120: both fades of a piece fit inside one frame

// |x| with NaN -> 0 (wave_abs of join.hip)
__device__ __forceinline__ float gate_abs(float x) {
    const float v = fabsf(x);
    return v == v ? v : 0.f;
}

// the samples of the segment from held_start on: [held (n_held) | chunk (n_new)]
struct gate_src {
    const float* held; const float* chunk; int held_start, n_held, n_new;
    __device__ __forceinline__ float at(int q) const { const int r = q - held_start; return r < n_held ? held[r] : chunk[r - n_held]; }
    // samples q .. q + n - 1 as one run of one buffer, or nullptr when they straddle the two
    __device__ __forceinline__ const float* run(int q, int n) const {
        const int r = q - held_start;
        return r + n <= n_held ? held + r : (r >= n_held ? chunk + (r - n_held) : nullptr);
    }
};

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// peak of frame f, wave-uniform: 16-byte loads where the frame is whole, lies in one buffer and starts on a 16-byte boundary
__device__ __forceinline__ float gate_frame_peak(const gate_src& s, int n_tot, int f, int lane) {
    const int q0 = f * GATE_FRAME, len = min(GATE_FRAME, n_tot - q0);
    const float* p = len == GATE_FRAME ? s.run(q0, GATE_FRAME) : nullptr;
    float m = 0.f;
    if (p && aligned16(p)) {
        if (lane < GATE_FRAME / 4) {
            const float4 v = reinterpret_cast<const float4*>(p)[lane];
            m = fmaxf(fmaxf(gate_abs(v.x), gate_abs(v.y)), fmaxf(gate_abs(v.z), gate_abs(v.w)));
        }
    } else {
        for (int q = lane; q < len; q += 64) m = fmaxf(m, gate_abs(s.at(q0 + q)));
    }
    return wave_max(m);
}

__device__ __forceinline__ int wave_min_i(int v) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// grid (1).  Frames f0 .. f1 - 1 of the segment; the values are >= 0 and never NaN, so fmaxf orders them as their bit patterns do.
__global__ __launch_bounds__(256) void k_wave_gate(cv2_wave_state* __restrict__ st, gate_src s, int f0, int f1, int seg_start, float g,
                                                   int32_t* __restrict__ record) {
    __shared__ float pk[GATE_TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n_tot = s.held_start + s.n_held + s.n_new;
    const uint32_t r_in = st->r_bits;
    const uint32_t c_bits = seg_start ? r_in : st->c_bits;                    // a new segment: C = the maximum over everything before it (R carries it: c_bits is kept for inspection only)
    int f_lo = seg_start ? -1 : st->f_lo, f_hi = seg_start ? -1 : st->f_hi;
    float R = __builtin_bit_cast(float, r_in);
    for (int t0 = f0; t0 < f1; t0 += GATE_TILE) {                             // (block-uniform)
        const int nt = min(GATE_TILE, f1 - t0);
        for (int j = w; j < nt; j += 4) {
            const float m = gate_frame_peak(s, n_tot, t0 + j, lane);
            if (lane == 0) pk[j] = m;
        }
        __syncthreads();
        if (w == 0) {                                                         // one wave: lane l holds frames 4 l .. 4 l + 3 of the tile
            float p[4], m = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                p[e] = 4 * lane + e < nt ? pk[4 * lane + e] : 0.f;
                m = fmaxf(m, p[e]);
            }
            float inc = m;                                                    // inclusive running maximum over the lanes
            for (int d = 1; d < 64; d <<= 1) {
                const float o = __shfl_up(inc, d);
                if (lane >= d) inc = fmaxf(inc, o);
            }
            const float before = __shfl_up(inc, 1);
            float run = lane == 0 ? R : fmaxf(R, before);
            int lo = INT_MAX, hi = -1;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (4 * lane + e < nt) {
                    run = fmaxf(run, p[e]);
                    const float thr = run * g;                                // the one fp32 product
                    if (run > 0.f && p[e] >= thr) { lo = min(lo, t0 + 4 * lane + e); hi = t0 + 4 * lane + e; }
                }
            }
            R = fmaxf(R, __shfl(inc, 63));
            lo = wave_min_i(lo);
            hi = wave_max_i(hi);
            if (hi >= 0) { if (f_lo < 0) f_lo = lo; f_hi = hi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {                                                   // (wave 0 holds R, f_lo, f_hi)
        const uint32_t r_bits = __builtin_bit_cast(uint32_t, R);
        st->r_bits = r_bits; st->c_bits = c_bits; st->frames = f1; st->f_lo = f_lo; st->f_hi = f_hi;
        record[0] = f_lo; record[1] = f_hi; record[2] = f1; record[3] = (int32_t)r_bits;
    }
}

static bool gate_disjoint(const void* a, long na, const void* b, long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na <= 0 || nb <= 0 || x + 4 * (uintptr_t)na <= y || y + 4 * (uintptr_t)nb <= x;
}

static int gate_check_src(const char* who, const float* held, int held_start, int n_held, const float* chunk, int n_new) {
    CV2_CHECK(held_start >= 0 && n_held >= 0 && n_new >= 0 && (long)held_start + n_held + n_new <= (1 << 30),
              "%s: held_start %d, %d held and %d new samples", who, held_start, n_held, n_new);
    CV2_CHECK(n_held == 0 || (held && ((uintptr_t)held & 3u) == 0), "%s: bad held buffer", who);
    CV2_CHECK(n_new == 0 || (chunk && ((uintptr_t)chunk & 3u) == 0), "%s: bad chunk", who);
    return 0;
}

extern "C" int cv2_wave_gate_chunk(cv2_wave_state* state_dev, const float* held, int32_t held_start, int32_t n_held, const float* chunk,
                                   int32_t n_new, int32_t f0, int32_t f1, int32_t seg_start, float g, int32_t* record_dev, void* stream) {
    CV2_CHECK(state_dev && record_dev && ((uintptr_t)state_dev & 3u) == 0 && ((uintptr_t)record_dev & 3u) == 0, "cv2_wave_gate_chunk: bad state or record");
    CV2_CHECK(g > 0.f && g <= 1.f, "cv2_wave_gate_chunk: g = %g outside (0, 1]", (double)g);
    if (gate_check_src("cv2_wave_gate_chunk", held, held_start, n_held, chunk, n_new)) return -1;
    const long n_tot = (long)held_start + n_held + n_new;
    CV2_CHECK(f0 >= 0 && f1 >= f0 && (long)GATE_FRAME * f0 >= held_start && (f1 == 0 || (long)GATE_FRAME * (f1 - 1) < n_tot),
              "cv2_wave_gate_chunk: frames %d .. %d of samples %d .. %ld", f0, f1, held_start, n_tot);
    const gate_src s{held, chunk, held_start, n_held, n_new};
    hipLaunchKernelGGL(k_wave_gate, dim3(1), dim3(256), 0, (hipStream_t)stream, state_dev, s, (int)f0, (int)f1, (int)seg_start, g, record_dev);
    CV2_LAUNCH_CHECK();
    return 0;
}

// elements by which the tile grid is shifted so that every group of four outputs starts on a 16-byte boundary (join_shift of join.hip)
__host__ __device__ __forceinline__ int emit_shift(const float* dst) { return (int)((reinterpret_cast<uintptr_t>(dst) & 15u) >> 2); }

// dst[o] = the segment's sample q0 + o for o < n_copy (times its fade weight inside a fade), +0.0f for n_copy <= o < n_out
__device__ __forceinline__ void emit_region(const cv2_wave_emit& a, const gate_src& s, float* __restrict__ dst, int n_out, int n_copy, int q0,
                                            bool fades) {
    const int sh = emit_shift(dst);
    const int tq = blockIdx.x * EMIT_TO + 4 * (int)threadIdx.x - sh;          // the thread's four consecutive outputs tq .. tq + 3
    if (tq + 3 < 0 || tq >= n_out) return;
    const int fi = fades ? a.fade_in_at : -1, fo = fades ? a.fade_out_end : -1, F = a.F;
    const bool full = tq >= 0 && tq + 4 <= n_out;                             // a whole group: aligned by the choice of the shift
    if (full && tq + 4 <= n_copy) {
        // the whole group inside one buffer, clear of both fades, and its source on a 16-byte boundary: one load, one store
        const int q = q0 + tq;
        const float* p = s.run(q, 4);
        const bool clear = (fi < 0 || q >= fi + F || q + 4 <= fi) && (fo < 0 || q + 4 <= fo - F || q >= fo);
        if (p && clear && aligned16(p)) {
            *reinterpret_cast<float4*>(dst + tq) = *reinterpret_cast<const float4*>(p);
            return;
        }
    }
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int o = tq + e;
        float x = 0.f;
        if (o >= 0 && o < n_copy) {
            const int q = q0 + o;
            x = s.at(q);
            if (fi >= 0 && q >= fi && q < fi + F) x *= a.fade_table[q - fi];
            else if (fo >= 0 && q >= fo - F && q < fo) x *= a.fade_table[fo - 1 - q];
        }
        v[e] = x;
    }
    if (full) {
        *reinterpret_cast<float4*>(dst + tq) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < 4; e++)
            if (tq + e >= 0 && tq + e < n_out) dst[tq + e] = v[e];
    }
}

// grid (blocks, 2): y = 0 writes the chunk's destination [samples e0 .. e1 - 1 | n_zero zeros], y = 1 the samples from keep_from on into
// held_dst (another buffer than held: nothing is moved in place)
__global__ __launch_bounds__(256) void k_wave_emit(cv2_wave_state* __restrict__ st, cv2_wave_emit a) {
    const gate_src s{a.held, a.chunk, a.held_start, a.n_held, a.n_new};
    const int n_keep = a.held_start + a.n_held + a.n_new - a.keep_from;
    if (blockIdx.y == 0) {
        emit_region(a, s, a.dst, a.e1 - a.e0 + a.n_zero, a.e1 - a.e0, a.e0, true);
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->n_held = n_keep; st->held_start = a.keep_from; }
    } else {
        emit_region(a, s, a.held_dst, n_keep, n_keep, a.keep_from, false);
    }
}

extern "C" int cv2_wave_emit_chunk(cv2_wave_state* state_dev, const cv2_wave_emit* a, void* stream) {
    CV2_CHECK(state_dev && a && ((uintptr_t)state_dev & 3u) == 0, "cv2_wave_emit_chunk: bad argument");
    if (gate_check_src("cv2_wave_emit_chunk", a->held, a->held_start, a->n_held, a->chunk, a->n_new)) return -1;
    const long n_tot = (long)a->held_start + a->n_held + a->n_new;
    CV2_CHECK(a->held_start <= a->e0 && a->e0 <= a->e1 && a->e1 <= a->keep_from && a->keep_from <= n_tot,
              "cv2_wave_emit_chunk: emits %d .. %d and keeps from %d on, of samples %d .. %ld", a->e0, a->e1, a->keep_from, a->held_start, n_tot);
    CV2_CHECK(a->n_zero >= 0 && a->n_zero <= (1 << 24), "cv2_wave_emit_chunk: n_zero = %d", a->n_zero);
    CV2_CHECK(a->F >= 0 && a->F <= MAX_FADE, "cv2_wave_emit_chunk: F = %d outside 0 .. %d", a->F, MAX_FADE);
    const long n_dst = (long)a->e1 - a->e0 + a->n_zero, n_keep = n_tot - a->keep_from;
    CV2_CHECK(n_dst == 0 || (a->dst && ((uintptr_t)a->dst & 3u) == 0), "cv2_wave_emit_chunk: bad destination");
    CV2_CHECK(n_keep <= a->held_cap && (n_keep == 0 || (a->held_dst && ((uintptr_t)a->held_dst & 3u) == 0)),
              "cv2_wave_emit_chunk: %ld samples stay held, the buffer takes %d", n_keep, a->held_cap);
    CV2_CHECK(gate_disjoint(a->held_dst, n_keep, a->held, a->n_held) && gate_disjoint(a->held_dst, n_keep, a->chunk, a->n_new) &&
              gate_disjoint(a->dst, n_dst, a->held, a->n_held) && gate_disjoint(a->dst, n_dst, a->chunk, a->n_new) &&
              gate_disjoint(a->dst, n_dst, a->held_dst, n_keep), "cv2_wave_emit_chunk: destination, held buffers and chunk overlap");
    CV2_CHECK(a->fade_in_at >= -1 && a->fade_out_end >= -1, "cv2_wave_emit_chunk: fades at %d / %d", a->fade_in_at, a->fade_out_end);
    if (a->F > 0 && (a->fade_in_at >= 0 || a->fade_out_end >= 0))
        CV2_CHECK(a->fade_table && ((uintptr_t)a->fade_table & 3u) == 0, "cv2_wave_emit_chunk: no fade table");
    if (a->fade_out_end >= 0) {                                               // the tail fade ends the emission and lies inside it
        CV2_CHECK(a->fade_out_end == a->e1 && a->e1 - a->F >= a->e0, "cv2_wave_emit_chunk: a tail fade of %d samples up to %d in an emission %d .. %d",
                  a->F, a->fade_out_end, a->e0, a->e1);
        CV2_CHECK(a->fade_in_at < 0 || a->fade_in_at + a->F <= a->fade_out_end - a->F, "cv2_wave_emit_chunk: the fades overlap");
    }
    const long longest = n_dst > n_keep ? n_dst : n_keep;
    const int blocks = (int)((longest + 3 + EMIT_TO - 1) / EMIT_TO);          // (+ 3: the largest shift)
    hipLaunchKernelGGL(k_wave_emit, dim3(blocks > 0 ? blocks : 1, 2), dim3(256), 0, (hipStream_t)stream, state_dev, *a);
    CV2_LAUNCH_CHECK();
    return 0;
}
