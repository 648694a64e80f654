// Output level of a call (an extension of the reference): a fixed gain, an optional scaling of the call's peak to a
// target, and a look-ahead limiter under a ceiling, on the device, ahead of the output stage (output.hip) and the device-to-host copy.
// Like the resampler it is defined on the GLOBAL sample index of the call, so a stream's chunks concatenate to exactly the levelling of
// the whole signal, bit for bit, wherever the chunk boundaries fell.  Everything is fp32 at 24 kHz; s[0 .. N) is the call's signal.
//
//   x[n] = Ge s[n]                      a[n] = |x[n]| (NaN counts as 0)
//   r[n] = a[n] > c ? c / a[n] : 1      d[n] = a[n] > c ? 1 - r[n] : 0                 (one correctly rounded division, one subtraction)
//   D[n] = max d[k], k = n .. min(n + L, N - 1)                                        (the look-ahead window)
//   acc[n] = sum_{j = 0 .. L, n - j >= 0} w[j] D[n - j]                                (ONE fmaf chain in ascending j from 0.f)
//   g[n] = max(0, min(1 - acc[n], r[n]))      y[n] = clamp(g[n] x[n], -c, c);   NaN x -> +0, infinite x -> +-c
//
// The chain sums the REDUCTIONS 1 - r, so wherever no sample within +-L is over the ceiling acc is exactly 0, g exactly 1 and (with Ge = 1)
// y[n] is s[n] bit for bit.  d is never negative and never NaN and w >= 0, so a partial sum is never -0: a tap before the signal's start
// may be multiplied by a D set to zero instead of being skipped, to the same bits.  The source samples first .. n_avail - 1 come as two
// pieces, the tail the call retained from earlier chunks and the chunk's new samples; which samples a chunk emits and which are retained is
// planned on the host in integers (cv2amd/level.py); the entry points check every range before they launch.
#include "common.h"
#include "../../include/cv2_amd.h"

constexpr int LV_TO = 1024;                             // outputs per block: 256 threads x 4 consecutive outputs
constexpr int LV_LMAX = 240;                            // longest look-ahead (10 ms)
constexpr int LV_LMIN = 24;
constexpr int LV_SPAN = LV_TO + 2 * LV_LMAX;            // source samples a block stages: its outputs and L on either side (3 x 5.9 KB of LDS)
constexpr int PK_TILE = 4096;                           // samples per block of the peak kernel: 256 threads x 4 x 16 bytes

// elements by which the tile grid is shifted so that every group of four outputs starts on a 16-byte boundary (out_shift of output.hip)
__host__ __device__ __forceinline__ int lv_shift(const float* dst) { return (int)((reinterpret_cast<uintptr_t>(dst) & 15u) >> 2); }

// 16-byte loads where the source allows them: scalar up to the next 16-byte boundary, float4 from there, scalar for what is left
__device__ __forceinline__ void lv_stage(const float* __restrict__ src, int n, float* __restrict__ dst, int tid, int nthr) {
    if (n <= 0) return;
    const int head = min(n, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2);
    const int nv = (n - head) >> 2;
    for (int i = tid; i < head; i += nthr) dst[i] = src[i];
    const float4* v = reinterpret_cast<const float4*>(src + head);
    for (int i = tid; i < nv; i += nthr) {
        const float4 q = v[i];
        float* d = dst + head + 4 * i;
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
    for (int i = head + 4 * nv + tid; i < n; i += nthr) dst[i] = src[i];
}

// |x| with NaN -> 0
__device__ __forceinline__ float lv_abs(float x) {
    const float v = fabsf(x);
    return v == v ? v : 0.f;
}

// Ge of a call: the record's gain, times T / P when the call is scaled to a peak target (P read from device memory: no host synchronisation)
__device__ __forceinline__ float lv_gain(const cv2_level_args& a) {
    if (a.peak == nullptr) return a.Ge;
    const float P = *a.peak;
    return P > 0.f ? __fmul_rn(a.Ge, __fdiv_rn(a.T, P)) : a.Ge;
}

// grid (ceil((max n_emit + shift) / 1024), 1, calls).  tab: device table of per-call records (one per blockIdx.z), or null: `one`.
__global__ __launch_bounds__(256) void k_level(const cv2_level_args* __restrict__ tab, cv2_level_args one) {
    __shared__ float xs[LV_SPAN];                                             // the source samples of the window
    __shared__ float ma[LV_SPAN], mb[LV_SPAN];                                // d, then the running window maxima (two buffers that take turns)
    __shared__ float ws[LV_LMAX + 1];
    const cv2_level_args a = tab ? tab[blockIdx.z] : one;
    const int tid = threadIdx.x, L = a.L;
    const int sh = lv_shift(a.dst);                                           // group g of the block covers outputs u - sh, u = 4 g .. 4 g + 3
    const int u0 = blockIdx.x * LV_TO;
    if (max(u0 - sh, 0) >= min(u0 + LV_TO - sh, a.n_emit)) return;            // no output of this call in the block (block-uniform)
    // the window: LDS index i holds global sample w_lo + i, i = 0 .. span - 1; thread t's outputs are the indices L + 4 t .. L + 4 t + 3.
    // Samples before 0 or from n_avail on (a final chunk: the signal's end; else no emitted output's window reaches them: checked) are 0.
    const int w_lo = a.n0 + u0 - sh - L, span = LV_TO + 2 * L;
    const int g_lo = max(w_lo, a.first), g_hi = min(w_lo + span, a.n_avail); // samples g_lo .. g_hi - 1 exist
    for (int i = tid; i < span; i += 256) {
        const int m = w_lo + i;
        if (m < g_lo || m >= g_hi) xs[i] = 0.f;
    }
    if (g_lo < g_hi) {
        // [g_lo, tail_end) lies in the retained tail, the rest in the new samples
        const int tail_end = a.first + a.n_tail;
        const int n_from_tail = max(0, min(g_hi, tail_end) - g_lo);
        if (n_from_tail > 0) lv_stage(a.tail + (g_lo - a.first), n_from_tail, xs + (g_lo - w_lo), tid, 256);
        const int f0 = max(g_lo, tail_end);
        lv_stage(a.fresh + (f0 - tail_end), g_hi - f0, xs + (f0 - w_lo), tid, 256);
    }
    for (int j = tid; j <= L; j += 256) ws[j] = a.weights[j];
    const float Ge = lv_gain(a), c = a.c;
    __syncthreads();
    // d, once per sample
    for (int i = tid; i < span; i += 256) {
        const float av = lv_abs(__fmul_rn(Ge, xs[i]));
        ma[i] = av > c ? __fsub_rn(1.f, __fdiv_rn(c, av)) : 0.f;
    }
    __syncthreads();
    // D[i] = max d[i .. i + L] by doubling: M_1 = d, M_2k[i] = max(M_k[i], M_k[i + k]) up to the largest power of two p <= L + 1, then
    // D[i] = max(M_p[i], M_p[i + L + 1 - p]) (the two runs overlap and cover the window); beyond the window's end there is nothing (d >= 0)
    float* cur = ma;
    float* nxt = mb;
    int k = 1;
    for (; 2 * k <= L + 1; k *= 2) {
        for (int i = tid; i < span; i += 256) nxt[i] = fmaxf(cur[i], i + k < span ? cur[i + k] : 0.f);
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
    }
    {
        const int off = L + 1 - k;
        // (D before the signal's start is set to 0: the chain multiplies such a tap by it instead of skipping it, to the same bits)
        for (int i = tid; i < span; i += 256) nxt[i] = w_lo + i >= 0 ? fmaxf(cur[i], i + off < span ? cur[i + off] : 0.f) : 0.f;
        __syncthreads();
    }
    const float* __restrict__ Dm = nxt;
    const int tq = u0 + 4 * tid - sh;                                         // the thread's four consecutive outputs tq .. tq + 3
    if (tq + 3 < 0 || tq >= a.n_emit) return;
    // the four chains side by side: step j reads D[i0 - j] anew, the other three operands slide along
    const int i0 = L + 4 * tid;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    float d1 = Dm[i0 + 1], d2 = Dm[i0 + 2], d3 = Dm[i0 + 3];
    for (int j = 0; j <= L; j++) {
        const float wj = ws[j], d0 = Dm[i0 - j];
        acc0 = fmaf(wj, d0, acc0);
        acc1 = fmaf(wj, d1, acc1);
        acc2 = fmaf(wj, d2, acc2);
        acc3 = fmaf(wj, d3, acc3);
        d3 = d2; d2 = d1; d1 = d0;
    }
    const float acc[4] = {acc0, acc1, acc2, acc3};
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float x = __fmul_rn(Ge, xs[i0 + e]);
        const float av = lv_abs(x);
        const float r = av > c ? __fdiv_rn(c, av) : 1.f;
        const float g = fmaxf(0.f, fminf(__fsub_rn(1.f, acc[e]), r));
        float y = fminf(fmaxf(__fmul_rn(g, x), -c), c);
        if (!(x == x)) y = 0.f;
        else if (av == INFINITY) y = copysignf(c, x);
        v[e] = y;
    }
    if (tq >= 0 && tq + 4 <= a.n_emit) {                                      // a whole group: aligned by the choice of the shift
        *reinterpret_cast<float4*>(a.dst + tq) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < 4; e++)
            if (tq + e >= 0 && tq + e < a.n_emit) a.dst[tq + e] = v[e];
    }
}

static int lv_check(const cv2_level_args& a, int z) {
    CV2_CHECK(a.L >= LV_LMIN && a.L <= LV_LMAX, "cv2_level_chunk: call %d: look-ahead of %d samples outside %d .. %d", z, a.L, LV_LMIN, LV_LMAX);
    CV2_CHECK(a.c > 0.f && a.c <= 1.f, "cv2_level_chunk: call %d: ceiling %g outside (0, 1]", z, (double)a.c);
    CV2_CHECK(a.Ge > 0.f && a.Ge <= 16.f, "cv2_level_chunk: call %d: gain %g outside (0, 16]", z, (double)a.Ge);
    CV2_CHECK(a.peak == nullptr || (a.T > 0.f && a.T <= a.c && ((uintptr_t)a.peak & 3u) == 0), "cv2_level_chunk: call %d: bad peak target", z);
    CV2_CHECK(a.weights && ((uintptr_t)a.weights & 3u) == 0, "cv2_level_chunk: call %d: no weight table", z);
    CV2_CHECK(a.first >= 0 && a.n_tail >= 0 && a.n_avail >= a.first + a.n_tail && a.n_avail <= (1 << 30), "cv2_level_chunk: call %d: bad sample counts", z);
    CV2_CHECK(a.n_final == -1 || a.n_final == a.n_avail, "cv2_level_chunk: call %d: n_final %d is neither -1 nor n_available %d", z, a.n_final, a.n_avail);
    CV2_CHECK(a.peak == nullptr || a.n_final >= 0, "cv2_level_chunk: call %d: a peak target needs the whole signal", z);
    const int n_new = a.n_avail - a.first - a.n_tail;
    CV2_CHECK((a.n_tail == 0 || a.tail) && (n_new == 0 || a.fresh), "cv2_level_chunk: call %d: bad source", z);
    CV2_CHECK(((uintptr_t)a.tail & 3u) == 0 && ((uintptr_t)a.fresh & 3u) == 0, "cv2_level_chunk: call %d: misaligned source", z);
    const long n_end = (long)a.n0 + a.n_emit;
    CV2_CHECK(a.n0 >= 0 && a.n_emit >= 0 && n_end <= (1 << 30), "cv2_level_chunk: call %d: bad output range", z);
    CV2_CHECK(a.n_emit <= a.dst_cap, "cv2_level_chunk: call %d: %d samples do not fit a destination of %d", z, a.n_emit, a.dst_cap);
    if (a.n_emit > 0) {
        CV2_CHECK(a.dst && ((uintptr_t)a.dst & 3u) == 0, "cv2_level_chunk: call %d: bad destination", z);
        // every sample an output reads is one of first .. n_available - 1 (a final chunk: the window ends with the signal)
        const int lo = a.n0 > a.L ? a.n0 - a.L : 0;
        CV2_CHECK(lo >= a.first, "cv2_level_chunk: call %d: output %d needs sample %d, retained from %d on", z, a.n0, lo, a.first);
        if (a.n_final < 0)
            CV2_CHECK(n_end - 1 + a.L <= (long)a.n_avail - 1, "cv2_level_chunk: call %d: output %ld looks ahead beyond the %d available", z, n_end - 1, a.n_avail);
        else
            CV2_CHECK(n_end <= a.n_final, "cv2_level_chunk: call %d: output %ld is beyond the signal's %d samples", z, n_end - 1, a.n_final);
    }
    return 0;
}

static inline int lv_blocks(const cv2_level_args& a) { return a.n_emit > 0 ? (a.n_emit + lv_shift(a.dst) + LV_TO - 1) / LV_TO : 0; }

extern "C" int cv2_level_chunk(const cv2_level_args* a, void* stream) {
    CV2_CHECK(a, "cv2_level_chunk: bad argument");
    if (lv_check(*a, 0)) return -1;
    if (a->n_emit == 0) return 0;
    hipLaunchKernelGGL(k_level, dim3(lv_blocks(*a), 1, 1), dim3(256), 0, (hipStream_t)stream, (const cv2_level_args*)nullptr, *a);
    CV2_LAUNCH_CHECK();
    return 0;
}

extern "C" int cv2_level_chunk_batch(const cv2_level_args* args, const cv2_level_args* table_dev, int32_t n, void* stream) {
    CV2_CHECK(args && table_dev && n >= 1 && n <= 65535 && ((uintptr_t)table_dev & 7u) == 0, "cv2_level_chunk_batch: bad argument");
    int blocks = 0;
    for (int z = 0; z < n; z++) {
        if (lv_check(args[z], z)) return -1;
        blocks = lv_blocks(args[z]) > blocks ? lv_blocks(args[z]) : blocks;
    }
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(k_level, dim3(blocks, 1, n), dim3(256), 0, (hipStream_t)stream, table_dev, args[0]);
    CV2_LAUNCH_CHECK();
    return 0;
}

// grid (ceil(max n / 4096), calls).  peaks[z] (zeroed ahead of the launch) receives P_z = max |s|: the values are >= 0, so their bit
// patterns order as unsigned integers and an integer atomicMax serves (k_wave_peak's rule); one atomic per block.
__global__ __launch_bounds__(256) void k_level_peak(const cv2_wave_seg* __restrict__ segs, unsigned* __restrict__ peaks) {
    __shared__ float sm[4];
    const cv2_wave_seg s = segs[blockIdx.y];
    const int q0 = blockIdx.x * PK_TILE;
    if (q0 >= s.n) return;                                                    // (block-uniform)
    const float* __restrict__ src = s.src + q0;
    const int n = min(PK_TILE, s.n - q0), tid = threadIdx.x;
    const int head = min(n, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2);
    const int nv = (n - head) >> 2;
    float m = 0.f;
    for (int i = tid; i < head; i += 256) m = fmaxf(m, lv_abs(src[i]));
    const float4* v = reinterpret_cast<const float4*>(src + head);
    for (int i = tid; i < nv; i += 256) {
        const float4 q = v[i];
        m = fmaxf(m, fmaxf(fmaxf(lv_abs(q.x), lv_abs(q.y)), fmaxf(lv_abs(q.z), lv_abs(q.w))));
    }
    for (int i = head + 4 * nv + tid; i < n; i += 256) m = fmaxf(m, lv_abs(src[i]));
    m = wave_max(m);
    if ((tid & 63) == 0) sm[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        if (m > 0.f) atomicMax(&peaks[blockIdx.y], __builtin_bit_cast(unsigned, m));
    }
}

extern "C" int cv2_level_peak_batch(const cv2_wave_seg* segs, const cv2_wave_seg* segs_dev, int32_t n, float* peaks_dev, void* stream) {
    CV2_CHECK(segs && segs_dev && peaks_dev && n >= 1 && n <= 65535, "cv2_level_peak_batch: bad argument (n = %d)", n);
    CV2_CHECK(((uintptr_t)peaks_dev & 3u) == 0 && ((uintptr_t)segs_dev & 7u) == 0, "cv2_level_peak_batch: misaligned table");
    int n_max = 0;
    for (int i = 0; i < n; i++) {
        CV2_CHECK(segs[i].n >= 0 && segs[i].n <= (1 << 30), "cv2_level_peak_batch: call %d: length %d", i, segs[i].n);
        CV2_CHECK(segs[i].n == 0 || (segs[i].src && ((uintptr_t)segs[i].src & 3u) == 0), "cv2_level_peak_batch: call %d: bad source", i);
        n_max = segs[i].n > n_max ? segs[i].n : n_max;
    }
    CV2_HIP(hipMemsetAsync(peaks_dev, 0, sizeof(float) * (size_t)n, (hipStream_t)stream));
    if (n_max == 0) return 0;
    hipLaunchKernelGGL(k_level_peak, dim3((n_max + PK_TILE - 1) / PK_TILE, n), dim3(256), 0, (hipStream_t)stream, segs_dev,
                       reinterpret_cast<unsigned*>(peaks_dev));
    CV2_LAUNCH_CHECK();
    return 0;
}
