// Integrated loudness of a call (ITU-R BS.1770-4: K-weighting, 400 ms blocks, an absolute and a relative gate), measured on the device so
// that a call can be scaled to a loudness target without its audio leaving the device (an extension of the reference).
//
// s[0 .. N) is the call's 24 kHz fp32 signal as it enters the level stage: after fade, trim and join, before gain_db, the limiter and the
// output conversion.  A non-finite sample counts as 0.
//   K-weighting: two biquads in cascade, the shelf, then the high-pass; coefficients computed on the host in float64 for fs = 24000 from
//     the analog prototype that reproduces the BS.1770 table at 48 kHz, K = tan(pi f0 / fs), a0 = 1 + K / Q + K^2:
//     shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G / 20), Vb = Vh^0.4996667741545416
//                b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
//     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773:  b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
//   Blocks: hop = 2400 samples (100 ms); block j covers y[2400 j .. 2400 j + 9600), j = 0 .. J - 1, J = floor((N - 9600) / 2400) + 1 when
//     N >= 9600, else 0; a tail shorter than a hop belongs to no block.  z_j = mean of y^2 over block j, l_j = -0.691 + 10 log10 z_j.
//   Gates: A = {j : l_j > -70};  Gamma = -0.691 + 10 log10 mean_A z_j - 10;  B = {j in A : l_j > Gamma};  z = mean_B z_j.
//   Lk = -0.691 + 10 log10 z.  No block, or A empty: Lk = -inf and the reference amplitude R is 0 (lv_gain of level.hip then leaves the
//     call's gain as it is).
//   Gain: T = float32(10^((loudness_lufs + 0.691) / 20)), R = sqrt(z) clamped to [T / g_max, T g_max], g_max = float32(10^(24 / 20)) (the
//     +-24 dB of gain_db).  R and Lk go to device memory; k_level runs with peak = &R and T: its Ge T / P is the loudness gain.
//
// The filter is a linear recurrence over a 4-value state (two biquads in transposed direct form II), so the unit of work is the hop:
//   pass 1   every hop runs from zero state -> its zero-state end state
//   scan     in hop order: s_start[h + 1] = M s_start[h] + zs_end[h], M = A^2400 (host, float64, rounded once), s_start[0] = 0
//   pass 2   every hop reruns from its true start state and sums y^2, one fmaf chain in sample order
//   finish   per call: block means and gates; the sums over blocks in a fixed order (thread t takes j = t, t + 256, ...; a fixed tree)
// Every value is a function of the call's samples alone: no atomics, no order that depends on the grid, on the other calls of the launch
// or on where a buffer lies.  The gates compare z_j, not l_j (z_j > 10^-6.9309 and z_j > mean_A / 10: the same sets).
#include "common.h"
#include "../../include/cv2_amd.h"

constexpr int LD_HOP = 2400;                            // samples per hop
constexpr int LD_GH = 8;                                // hops per workgroup of the two passes, one lane each
constexpr int LD_ROW = LD_HOP + 1;                      // LDS floats per hop: an odd stride, lane h reads bank (h + i) % 32
constexpr int LD_SC = 256;                              // hops the scan stages at a time

__host__ __device__ __forceinline__ int ld_hops(int n) { return n >= 4 * LD_HOP ? n / LD_HOP : 0; }      // the hops that lie in a block

struct ld_ws {                                          // the caller's scratch: [calls][nh_max] records each
    float* zs;                                          // 4 floats: zero-state end state of the hop
    float* st;                                          // 4 floats: true start state of the hop
    float* e;                                           // 1 float: sum of y^2 over the hop
};
static inline size_t ld_ws_floats(size_t n, size_t nh_max) { return n * nh_max * 9; }
static inline ld_ws ld_carve(void* ws, size_t n, size_t nh_max) {
    float* p = static_cast<float*>(ws);
    return ld_ws{p, p + n * nh_max * 4, p + n * nh_max * 8};
}

// one sample through the cascade; the state is (s1, s2) of the shelf and (t1, t2) of the high-pass.  f: b0 b1 b2 a1 a2 | c1 c2
__device__ __forceinline__ float ld_step(const float (&f)[7], float x, float (&s)[4]) {
    const float y = fmaf(f[0], x, s[0]);
    s[0] = fmaf(-f[3], y, fmaf(f[1], x, s[1]));
    s[1] = fmaf(-f[4], y, __fmul_rn(f[2], x));
    const float w = __fadd_rn(y, s[2]);
    s[2] = fmaf(-f[5], w, fmaf(-2.f, y, s[3]));
    s[3] = fmaf(-f[6], w, y);
    return w;
}

// grid (ceil(nh_max / 8), calls).  PASS 1: zs[h] = end state from zero state.  PASS 2: e[h] = sum y^2 from the start state st[h].
template <int PASS>
__global__ __launch_bounds__(256) void k_loud_pass(const cv2_wave_seg* __restrict__ segs, const float* __restrict__ filt, ld_ws ws, int nh_max) {
    __shared__ float xs[LD_GH * LD_ROW];
    const cv2_wave_seg sg = segs[blockIdx.y];
    const int nh = ld_hops(sg.n), h0 = blockIdx.x * LD_GH, tid = threadIdx.x;
    if (h0 >= nh) return;                                                     // (block-uniform)
    const int gh = min(LD_GH, nh - h0), cnt = gh * LD_HOP;
    // the block's samples h0 * 2400 .. + cnt: 16-byte loads where the source allows them; sample i of the range goes to xs[i + i / 2400]
    const float* __restrict__ src = sg.src + (size_t)h0 * LD_HOP;
    const int head = min(cnt, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2);
    const int nv = (cnt - head) >> 2;
    for (int i = tid; i < head; i += 256) {
        const float v = src[i];
        xs[i] = fabsf(v) < INFINITY ? v : 0.f;                                // (head < 4: the first hop)
    }
    const float4* v4 = reinterpret_cast<const float4*>(src + head);
    for (int q = tid; q < nv; q += 256) {
        const float4 v = v4[q];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = head + 4 * q + k;
            xs[i + i / LD_HOP] = fabsf(e[k]) < INFINITY ? e[k] : 0.f;
        }
    }
    for (int i = head + 4 * nv + tid; i < cnt; i += 256) {
        const float v = src[i];
        xs[i + i / LD_HOP] = fabsf(v) < INFINITY ? v : 0.f;
    }
    __syncthreads();
    if (tid >= gh) return;
    float f[7];
#pragma unroll
    for (int k = 0; k < 7; k++) f[k] = filt[k];
    const size_t rec = (size_t)blockIdx.y * nh_max + h0 + tid;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (PASS == 2) {
        const float4 q = *reinterpret_cast<const float4*>(ws.st + 4 * rec);
        s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
    }
    const float* __restrict__ x = xs + tid * LD_ROW;
    float e = 0.f;
#pragma unroll 8
    for (int i = 0; i < LD_HOP; i++) {
        const float w = ld_step(f, x[i], s);
        if (PASS == 2) e = fmaf(w, w, e);
    }
    if (PASS == 1) *reinterpret_cast<float4*>(ws.zs + 4 * rec) = make_float4(s[0], s[1], s[2], s[3]);
    else ws.e[rec] = e;
}

// grid (calls), 64 threads.  st[0] = 0, st[h + 1] = M st[h] + zs[h], row i as ONE fmaf chain from zs[h][i] in ascending column order.
__global__ __launch_bounds__(64) void k_loud_scan(const cv2_wave_seg* __restrict__ segs, const float* __restrict__ filt, ld_ws ws, int nh_max) {
    __shared__ float4 buf[LD_SC];
    const int nh = ld_hops(segs[blockIdx.x].n), tid = threadIdx.x;
    const size_t rec0 = (size_t)blockIdx.x * nh_max;
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = filt[8 + k];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);                               // (lane 0's: the state at the start of hop h0)
    for (int h0 = 0; h0 < nh; h0 += LD_SC) {
        const int cnt = min(LD_SC, nh - h0);
        for (int k = tid; k < cnt; k += 64) buf[k] = *reinterpret_cast<const float4*>(ws.zs + 4 * (rec0 + h0 + k));
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < cnt; k++) {
                const float4 z = buf[k];
                buf[k] = s;
                float4 t;
                t.x = fmaf(M[3], s.w, fmaf(M[2], s.z, fmaf(M[1], s.y, fmaf(M[0], s.x, z.x))));
                t.y = fmaf(M[7], s.w, fmaf(M[6], s.z, fmaf(M[5], s.y, fmaf(M[4], s.x, z.y))));
                t.z = fmaf(M[11], s.w, fmaf(M[10], s.z, fmaf(M[9], s.y, fmaf(M[8], s.x, z.z))));
                t.w = fmaf(M[15], s.w, fmaf(M[14], s.z, fmaf(M[13], s.y, fmaf(M[12], s.x, z.w))));
                s = t;
            }
        }
        __syncthreads();
        for (int k = tid; k < cnt; k += 64) *reinterpret_cast<float4*>(ws.st + 4 * (rec0 + h0 + k)) = buf[k];
        __syncthreads();
    }
}

// mean of y^2 over block j: the four hop sums added in hop order in float64
__device__ __forceinline__ double ld_block(const float* __restrict__ e, int j) {
    return ((((double)e[j] + (double)e[j + 1]) + (double)e[j + 2]) + (double)e[j + 3]) / (4.0 * LD_HOP);
}

// fixed tree over the 256 partial sums and counts; the result in every thread
__device__ __forceinline__ void ld_tree(double* sm, int* cn, double& v, int& c, int tid) {
    __syncthreads();
    sm[tid] = v; cn[tid] = c;
    __syncthreads();
    for (int k = 128; k >= 1; k >>= 1) {
        if (tid < k) { sm[tid] += sm[tid + k]; cn[tid] += cn[tid + k]; }
        __syncthreads();
    }
    v = sm[0]; c = cn[0];
}

// grid (calls), 256 threads.  targets: T per call (0: R is not clamped) or null.
__global__ __launch_bounds__(256) void k_loud_finish(const cv2_wave_seg* __restrict__ segs, const float* __restrict__ targets, ld_ws ws, int nh_max,
                                                     float* __restrict__ R_out, float* __restrict__ lufs_out) {
    __shared__ double sm[256];
    __shared__ int cn[256];
    const int z = blockIdx.x, tid = threadIdx.x;
    const int nh = ld_hops(segs[z].n), J = nh > 0 ? nh - 3 : 0;
    const float* __restrict__ e = ws.e + (size_t)z * nh_max;
    const double gate_abs = 1.1724653045822981e-07;                           // 10^((-70 + 0.691) / 10)
    double v = 0.0;
    int c = 0;
    for (int j = tid; j < J; j += 256) {
        const double zj = ld_block(e, j);
        if (zj > gate_abs) { v += zj; c++; }
    }
    ld_tree(sm, cn, v, c, tid);
    float R = 0.f, lk = -INFINITY;
    if (c > 0) {                                                              // (block-uniform)
        const double gate_rel = v / (double)c * 0.1;
        v = 0.0; c = 0;
        for (int j = tid; j < J; j += 256) {
            const double zj = ld_block(e, j);
            if (zj > gate_abs && zj > gate_rel) { v += zj; c++; }
        }
        ld_tree(sm, cn, v, c, tid);
        const double zz = v / (double)c;                                      // (the loudest block of A is above the relative gate: c >= 1)
        lk = (float)(-0.691 + 10.0 * log10(zz));
        R = (float)sqrt(zz);
        const float T = targets ? targets[z] : 0.f;
        if (T > 0.f) {
            const float g_max = 15.848931924611133f;                          // float32(10^(24 / 20))
            R = fminf(fmaxf(R, __fdiv_rn(T, g_max)), __fmul_rn(T, g_max));
        }
    }
    if (tid == 0) { R_out[z] = R; lufs_out[z] = lk; }
}

static int ld_check(const cv2_wave_seg* segs, int32_t n, int* nh_max) {
    CV2_CHECK(segs && n >= 1 && n <= 65535, "cv2_loudness: bad argument (n = %d)", n);
    int m = 0;
    for (int i = 0; i < n; i++) {
        CV2_CHECK(segs[i].n >= 0 && segs[i].n <= (1 << 30), "cv2_loudness: call %d: length %d", i, segs[i].n);
        CV2_CHECK(segs[i].n == 0 || (segs[i].src && ((uintptr_t)segs[i].src & 3u) == 0), "cv2_loudness: call %d: bad source", i);
        m = ld_hops(segs[i].n) > m ? ld_hops(segs[i].n) : m;
    }
    *nh_max = m;
    return 0;
}

extern "C" int cv2_loudness_workspace_bytes(const cv2_wave_seg* segs, int32_t n, size_t* bytes) {
    int nh_max = 0;
    CV2_CHECK(bytes, "cv2_loudness_workspace_bytes: bad argument");
    if (ld_check(segs, n, &nh_max)) return -1;
    *bytes = (ld_ws_floats((size_t)n, (size_t)nh_max) * sizeof(float) + 15) & ~(size_t)15;
    return 0;
}

extern "C" int cv2_loudness_batch(const cv2_wave_seg* segs, const cv2_wave_seg* segs_dev, int32_t n, const float* targets, const float* targets_dev,
                                  const float* filter_dev, float* R_dev, float* lufs_dev, void* ws, size_t ws_bytes, void* stream) {
    int nh_max = 0;
    if (ld_check(segs, n, &nh_max)) return -1;
    CV2_CHECK(segs_dev && ((uintptr_t)segs_dev & 7u) == 0, "cv2_loudness_batch: no device table of the records");
    CV2_CHECK(filter_dev && ((uintptr_t)filter_dev & 3u) == 0, "cv2_loudness_batch: no filter table");
    CV2_CHECK(R_dev && lufs_dev && ((uintptr_t)R_dev & 3u) == 0 && ((uintptr_t)lufs_dev & 3u) == 0, "cv2_loudness_batch: bad result pointers");
    CV2_CHECK((targets == nullptr) == (targets_dev == nullptr) && ((uintptr_t)targets_dev & 3u) == 0, "cv2_loudness_batch: targets need a host and a device copy");
    if (targets)
        for (int i = 0; i < n; i++)
            CV2_CHECK(targets[i] >= 0.f && targets[i] <= 1.f, "cv2_loudness_batch: call %d: target %g outside [0, 1]", i, (double)targets[i]);
    const size_t need = ld_ws_floats((size_t)n, (size_t)nh_max) * sizeof(float);
    CV2_CHECK(need == 0 || (ws && ((uintptr_t)ws & 15u) == 0 && ws_bytes >= need), "cv2_loudness_batch: workspace of %zu bytes, %zu needed (16-byte aligned)",
              ws_bytes, need);
    const ld_ws w = ld_carve(ws, (size_t)n, (size_t)nh_max);
    hipStream_t st = (hipStream_t)stream;
    if (nh_max > 0) {
        const dim3 grid((nh_max + LD_GH - 1) / LD_GH, n);
        hipLaunchKernelGGL(k_loud_pass<1>, grid, dim3(256), 0, st, segs_dev, filter_dev, w, nh_max);
        CV2_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_loud_scan, dim3(n), dim3(64), 0, st, segs_dev, filter_dev, w, nh_max);
        CV2_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_loud_pass<2>, grid, dim3(256), 0, st, segs_dev, filter_dev, w, nh_max);
        CV2_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_loud_finish, dim3(n), dim3(256), 0, st, segs_dev, targets_dev, w, nh_max, R_dev, lufs_dev);
    CV2_LAUNCH_CHECK();
    return 0;
}
