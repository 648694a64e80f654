// Joined calls (an extension of the reference): the 24 kHz waveforms of one call's text segments, still on the
// device, written into ONE waveform -- interior silences optionally trimmed, a pause of zeros between the pieces, a short raised-cosine
// fade at each trimmed edge -- ahead of the output stage and the one device-to-host copy.
//
//   bounds (cv2_wave_bounds): frames of 240 samples, peak_f = max |s[q]| over the frame (NaN counts as 0), P = max_f peak_f,
//     thr = P * g (ONE fp32 product), frame f is loud iff P > 0 and peak_f >= thr; the kept range [a, b) reaches WAVE_KEEP samples
//     beyond the first / last loud frame at INTERIOR edges only.  Maxima and one rounded product: a host restatement gives the same integers.
//   join (cv2_wave_join): every output sample is a copy (bit for bit), a copy times one fade weight (one fp32 multiply), or +0.0f.
//
// Both are streaming kernels bound by memory bandwidth; the entry points check every range before they launch.
#include <limits.h>
#include "common.h"
#include "../../include/cv2_amd.h"

constexpr int WAVE_FRAME = 240;                         // samples per frame (10 ms at 24 kHz), no overlap
constexpr int WAVE_KEEP = 480;                          // samples kept beyond the first / last loud frame
constexpr int WAVE_TILE = 16;                           // frames per block: 4 waves x 4 frames
constexpr int JOIN_TO = 1024;                           // outputs per block: 256 threads x 4 consecutive outputs

// |x| with NaN -> 0
__device__ __forceinline__ float wave_abs(float x) {
    const float v = fabsf(x);
    return v == v ? v : 0.f;
}

// peak of frame f of one segment, wave-uniform: 16-byte loads where the segment allows them (a frame starts 960 f bytes into it)
__device__ __forceinline__ float wave_frame_peak(const float* __restrict__ src, int n, int f, int lane) {
    const int q0 = f * WAVE_FRAME, len = min(WAVE_FRAME, n - q0);
    float m = 0.f;
    if (len == WAVE_FRAME && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        if (lane < WAVE_FRAME / 4) {
            const float4 v = reinterpret_cast<const float4*>(src + q0)[lane];
            m = fmaxf(fmaxf(wave_abs(v.x), wave_abs(v.y)), fmaxf(wave_abs(v.z), wave_abs(v.w)));
        }
    } else {
        for (int q = lane; q < len; q += 64) m = fmaxf(m, wave_abs(src[q0 + q]));
    }
    return wave_max(m);
}

// grid (ceil(max frames / 16), k).  peaks[i] (zeroed ahead of the launch) receives P_i: the values are >= 0, so their bit patterns order
// as unsigned integers and an integer atomicMax serves.  Also arms bounds[i] for k_wave_loud.
__global__ __launch_bounds__(256) void k_wave_peak(const cv2_wave_seg* __restrict__ segs, unsigned* __restrict__ peaks, int* __restrict__ bounds) {
    __shared__ float sm[4];
    const int i = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const cv2_wave_seg s = segs[i];
    const int n_frames = (s.n + WAVE_FRAME - 1) / WAVE_FRAME, f0 = blockIdx.x * WAVE_TILE;
    if (blockIdx.x == 0 && threadIdx.x == 0) { bounds[2 * i] = INT_MAX; bounds[2 * i + 1] = -1; }
    if (f0 >= n_frames) return;                                               // (block-uniform)
    float m = 0.f;
    for (int f = f0 + w; f < min(f0 + WAVE_TILE, n_frames); f += 4) m = fmaxf(m, wave_frame_peak(s.src, s.n, f, lane));
    if (lane == 0) sm[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        if (m > 0.f) atomicMax(&peaks[i], __builtin_bit_cast(unsigned, m));
    }
}

// same grid, after k_wave_peak.  a = max(0, 240 f_lo - keep) and b = min(n, 240 (f_hi + 1) + keep) are monotone in the frame index, so
// every loud frame offers its own a and b: atomicMin / atomicMax on integers, whatever the order.
__global__ __launch_bounds__(256) void k_wave_loud(const cv2_wave_seg* __restrict__ segs, int k, float g, const float* __restrict__ peaks,
                                                   int* __restrict__ bounds) {
    const int i = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const cv2_wave_seg s = segs[i];
    const float P = peaks[i];
    if (!(P > 0.f)) {                                                         // a silent segment is kept whole
        if (blockIdx.x == 0 && threadIdx.x == 0) { bounds[2 * i] = 0; bounds[2 * i + 1] = s.n; }
        return;
    }
    const float thr = P * g;
    const int n_frames = (s.n + WAVE_FRAME - 1) / WAVE_FRAME, f0 = blockIdx.x * WAVE_TILE;
    int lo = INT_MAX, hi = -1;
    for (int f = f0 + w; f < min(f0 + WAVE_TILE, n_frames); f += 4)
        if (wave_frame_peak(s.src, s.n, f, lane) >= thr) { lo = min(lo, f); hi = max(hi, f); }
    if (lane == 0 && hi >= 0) {
        atomicMin(&bounds[2 * i], i > 0 ? max(0, WAVE_FRAME * lo - WAVE_KEEP) : 0);
        atomicMax(&bounds[2 * i + 1], i < k - 1 ? min(s.n, WAVE_FRAME * (hi + 1) + WAVE_KEEP) : s.n);
    }
}

extern "C" int cv2_wave_bounds(const cv2_wave_seg* segs, const cv2_wave_seg* segs_dev, int32_t k, float g, int32_t* bounds_dev, float* peaks_dev,
                               void* stream) {
    CV2_CHECK(segs && segs_dev && bounds_dev && peaks_dev && k >= 1 && k <= CV2_WAVE_MAX_PIECES, "cv2_wave_bounds: bad argument (k = %d)", k);
    CV2_CHECK(g > 0.f && g <= 1.f, "cv2_wave_bounds: g = %g outside (0, 1]", (double)g);
    CV2_CHECK(((uintptr_t)bounds_dev & 3u) == 0 && ((uintptr_t)peaks_dev & 3u) == 0 && ((uintptr_t)segs_dev & 7u) == 0, "cv2_wave_bounds: misaligned table");
    int n_max = 0;
    for (int i = 0; i < k; i++) {
        CV2_CHECK(segs[i].n >= 1 && segs[i].n <= (1 << 30), "cv2_wave_bounds: segment %d: length %d", i, segs[i].n);
        CV2_CHECK(segs[i].src && ((uintptr_t)segs[i].src & 3u) == 0, "cv2_wave_bounds: segment %d: bad source", i);
        n_max = segs[i].n > n_max ? segs[i].n : n_max;
    }
    const int frames = (n_max + WAVE_FRAME - 1) / WAVE_FRAME;
    const dim3 grid((frames + WAVE_TILE - 1) / WAVE_TILE, k, 1);
    CV2_HIP(hipMemsetAsync(peaks_dev, 0, sizeof(float) * (size_t)k, (hipStream_t)stream));
    hipLaunchKernelGGL(k_wave_peak, grid, dim3(256), 0, (hipStream_t)stream, segs_dev, reinterpret_cast<unsigned*>(peaks_dev), bounds_dev);
    CV2_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_wave_loud, grid, dim3(256), 0, (hipStream_t)stream, segs_dev, (int)k, g, (const float*)peaks_dev, bounds_dev);
    CV2_LAUNCH_CHECK();
    return 0;
}

// elements by which the tile grid is shifted so that every group of four outputs starts on a 16-byte boundary (out_shift of output.hip)
__host__ __device__ __forceinline__ int join_shift(const float* dst) { return (int)((reinterpret_cast<uintptr_t>(dst) & 15u) >> 2); }

// output o of the joined signal, given the last piece j (or -1) with dst_off <= o
__device__ __forceinline__ float join_sample(const cv2_wave_piece& p, int r, const float* __restrict__ fade, int F) {
    float v = p.src[p.src_off + r];
    if ((p.fade & CV2_WAVE_FADE_IN) && r < F) v *= fade[r];
    else if ((p.fade & CV2_WAVE_FADE_OUT) && r >= p.m - F) v *= fade[p.m - 1 - r];
    return v;
}

// grid (ceil((n_dst + shift) / 1024)).  Pieces in ascending dst_off, not overlapping; what no piece covers is +0.0f.
__global__ __launch_bounds__(256) void k_wave_join(const cv2_wave_piece* __restrict__ tab, int k, const float* __restrict__ fade, int F,
                                                   float* __restrict__ dst, int n_dst) {
    const int sh = join_shift(dst);
    const int u0 = blockIdx.x * JOIN_TO;
    // the last piece that starts at or before the block's first output (block-uniform search), -1: none
    int j = -1;
    {
        const int o_first = max(u0 - sh, 0);
        int lo = 0, hi = k;                                                   // pieces [0, lo) start at or before o_first, [hi, k) after it
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (tab[mid].dst_off <= o_first) lo = mid + 1; else hi = mid;
        }
        j = lo - 1;
    }
    const int tq = u0 + 4 * (int)threadIdx.x - sh;                            // the thread's four consecutive outputs tq .. tq + 3
    if (tq + 3 < 0 || tq >= n_dst) return;
    while (j + 1 < k && tab[j + 1].dst_off <= max(tq, 0)) j++;
    const bool full = tq >= 0 && tq + 4 <= n_dst;                             // a whole group: aligned by the choice of the shift
    if (full && j >= 0) {
        const cv2_wave_piece p = tab[j];
        const int r = tq - p.dst_off;
        // the whole group inside the piece, clear of both fades, and its source on a 16-byte boundary: one load, one store
        const float* s = p.src + p.src_off + r;
        const int f_in = (p.fade & CV2_WAVE_FADE_IN) ? F : 0, f_out = (p.fade & CV2_WAVE_FADE_OUT) ? F : 0;
        if (r + 4 <= p.m - f_out && r >= f_in && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
            *reinterpret_cast<float4*>(dst + tq) = *reinterpret_cast<const float4*>(s);
            return;
        }
    }
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int o = tq + e;
        float x = 0.f;
        if (o >= 0 && o < n_dst) {
            while (j + 1 < k && tab[j + 1].dst_off <= o) j++;
            if (j >= 0) {
                const cv2_wave_piece p = tab[j];
                if (o - p.dst_off < p.m) x = join_sample(p, o - p.dst_off, fade, F);
            }
        }
        v[e] = x;
    }
    if (full) {
        *reinterpret_cast<float4*>(dst + tq) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < 4; e++)
            if (tq + e >= 0 && tq + e < n_dst) dst[tq + e] = v[e];
    }
}

extern "C" int cv2_wave_join(const cv2_wave_piece* pieces, const cv2_wave_piece* pieces_dev, int32_t k, const float* fade_table_dev, int32_t F,
                             float* dst, int32_t n_dst, void* stream) {
    CV2_CHECK(pieces && pieces_dev && k >= 1 && k <= CV2_WAVE_MAX_PIECES, "cv2_wave_join: bad argument (k = %d)", k);
    CV2_CHECK(((uintptr_t)pieces_dev & 7u) == 0, "cv2_wave_join: misaligned table");
    CV2_CHECK(F >= 0 && F <= (1 << 20), "cv2_wave_join: F = %d", F);
    CV2_CHECK(n_dst >= 0 && n_dst <= (1 << 30), "cv2_wave_join: n_dst = %d", n_dst);
    CV2_CHECK(n_dst == 0 || (dst && ((uintptr_t)dst & 3u) == 0), "cv2_wave_join: bad destination");
    long end = 0;                                                             // end of the previous piece in the joined signal
    for (int i = 0; i < k; i++) {
        const cv2_wave_piece& p = pieces[i];
        CV2_CHECK(p.n_src >= 0 && p.n_src <= (1 << 30) && p.src_off >= 0 && p.m >= 0 && (long)p.src_off + p.m <= p.n_src,
                  "cv2_wave_join: piece %d: samples %d .. %ld of a source of %d", i, p.src_off, (long)p.src_off + p.m, p.n_src);
        CV2_CHECK(p.m == 0 || (p.src && ((uintptr_t)p.src & 3u) == 0), "cv2_wave_join: piece %d: bad source", i);
        CV2_CHECK(p.dst_off >= end, "cv2_wave_join: piece %d starts at %d, inside or before its predecessor (which ends at %ld)", i, p.dst_off, end);
        end = (long)p.dst_off + p.m;
        CV2_CHECK(end <= n_dst, "cv2_wave_join: piece %d ends at %ld, beyond the destination's %d samples", i, end, n_dst);
        CV2_CHECK((p.fade & ~(CV2_WAVE_FADE_IN | CV2_WAVE_FADE_OUT)) == 0, "cv2_wave_join: piece %d: fade flags %d", i, p.fade);
        if (p.fade && F > 0) {
            CV2_CHECK(p.m >= 2 * (long)F, "cv2_wave_join: piece %d: a fade of %d samples needs at least %d, the piece has %d", i, F, 2 * F, p.m);
            CV2_CHECK(fade_table_dev && ((uintptr_t)fade_table_dev & 3u) == 0, "cv2_wave_join: piece %d: no fade table", i);
        }
    }
    if (n_dst == 0) return 0;
    const int blocks = (n_dst + join_shift(dst) + JOIN_TO - 1) / JOIN_TO;
    hipLaunchKernelGGL(k_wave_join, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pieces_dev, (int)k, fade_table_dev, (int)F, dst, (int)n_dst);
    CV2_LAUNCH_CHECK();
    return 0;
}
