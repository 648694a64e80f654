// Output side of a call (an extension of the reference): the 24 kHz waveform of a call resampled to the rate the
// caller asked for and, optionally, converted to int16 PCM, on the device, before the device-to-host copy.  The resampling is the
// reference's own definition for prompts -- torchaudio's sinc_interp_hann polyphase convolution, k_resample in frontend.hip -- in a
// stateful form: the filter is defined on the GLOBAL sample index of the call, so a stream's chunks concatenate to exactly what
// cv2_resample gives for the whole signal, bit for bit, wherever the chunk boundaries fell.
//
//   o = i up + p (0 <= p < up):   y[o] = sum_{j = 0 .. klen - 1, 0 <= q < n} K[p][j] s[q],   q = i down - width + j
//
// one fp32 fmaf chain in ascending j from 0.f, taps outside the signal skipped (k_resample's order).  The source samples
// first .. n_avail - 1 come as two pieces: the tail the call retained from earlier chunks and the chunk's new samples.  Which outputs a
// chunk emits and which samples are retained is planned on the host in integers (cv2amd/outrate.py); the entry points check every range
// before they launch.
#include "common.h"
#include "../../include/cv2_amd.h"

constexpr int OUT_TO = 1024;                            // outputs per block: 256 threads x 4 consecutive outputs
constexpr int OUT_SPAN = 3584;                          // source samples a block can stage (14 KB of LDS): 8 kHz needs 3 * 1025 + 41

// source samples a tile of OUT_TO outputs (plus the alignment shift) can touch
static inline long out_span_need(int up, int down, int klen) { return ((long)(OUT_TO + 3 + up - 1) / up + 1) * down + klen; }

// elements by which the tile grid is shifted so that every group of four outputs starts on a 16-byte (float) / 8-byte (int16) boundary
__host__ __device__ __forceinline__ int out_shift(const void* dst, int format) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    return format == CV2_OUT_PCM16 ? (int)((a & 7u) >> 1) : (int)((a & 15u) >> 2);
}

// 16-byte loads where the source allows them: scalar up to the next 16-byte boundary, float4 from there, scalar for what is left
__device__ __forceinline__ void out_stage(const float* __restrict__ src, int n, float* __restrict__ dst, int tid, int nthr) {
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

// trunc_toward_zero(y * 32768) saturated to [-32768, 32767], NaN -> 0 (y * 32768 is exact: a power of two)
__device__ __forceinline__ short out_pcm16(float y) {
    const float v = y * 32768.f;
    if (!(v == v)) return 0;
    if (v >= 32767.f) return 32767;
    if (v <= -32768.f) return -32768;
    return (short)(int)v;
}

// grid (ceil((max n_emit + shift) / 1024), 1, calls).  tab: device table of per-call records (one per blockIdx.z), or null: `one`.
__global__ __launch_bounds__(256) void k_out_resample(const cv2_out_args* __restrict__ tab, cv2_out_args one) {
    __shared__ float sm[OUT_SPAN];
    const cv2_out_args a = tab ? tab[blockIdx.z] : one;
    const int sh = out_shift(a.dst, a.format);                                // group g of the block covers outputs u - sh, u = 4 g .. 4 g + 3
    const int u0 = blockIdx.x * OUT_TO;
    const int t_lo = max(u0 - sh, 0), t_hi = min(u0 + OUT_TO - sh, a.n_emit) - 1;       // the block's outputs, relative to o0
    if (t_lo > t_hi) return;                                                  // (block-uniform)
    // source window of the block: every in-range tap of its outputs
    const int i_lo = (a.o0 + t_lo) / a.up, i_hi = (a.o0 + t_hi) / a.up;
    const int q_lo = max(i_lo * a.down - a.width, a.first);
    const int q_hi = min(i_hi * a.down - a.width + a.klen - 1, a.n_avail - 1);
    const int span = min(q_hi - q_lo + 1, OUT_SPAN);                          // (the entry point has checked the rates and the sample ranges)
    {
        // samples q_lo .. q_lo + span - 1: [q_lo, tail_end) lies in the retained tail, the rest in the new samples
        const int tail_end = a.first + a.n_tail;
        const int n_from_tail = max(0, min(q_lo + span, tail_end) - q_lo);
        if (n_from_tail > 0) out_stage(a.tail + (q_lo - a.first), n_from_tail, sm, threadIdx.x, 256);
        const int f0 = max(q_lo, tail_end);
        out_stage(a.fresh + (f0 - tail_end), q_lo + span - f0, sm + (f0 - q_lo), threadIdx.x, 256);
    }
    __syncthreads();
    const int tq = u0 + 4 * (int)threadIdx.x - sh;                            // the thread's four consecutive outputs tq .. tq + 3
    if (tq + 3 < t_lo || tq > t_hi) return;
    const int tc = max(tq, 0);
    int i = (a.o0 + tc) / a.up, p = (a.o0 + tc) - i * a.up;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int t = tq + e;
        float s = 0.f;
        if (t >= 0 && t < a.n_emit) {
            const int base = i * a.down - a.width;
            if (a.kernel == nullptr) {
                s = sm[base - q_lo];                                          // 24 kHz: no filter, the sample itself
            } else {
                const float* __restrict__ kp = a.kernel + (size_t)p * a.klen;
                const int j0 = max(0, -base), j1 = min(a.klen, a.n_avail - base);
                const float* __restrict__ x = sm + (base - q_lo);
                for (int j = j0; j < j1; j++) s = fmaf(kp[j], x[j], s);
            }
            if (++p == a.up) { p = 0; i++; }
        }
        v[e] = s;
    }
    const bool full = tq >= 0 && tq + 4 <= a.n_emit;                          // a whole group: aligned by the choice of the shift
    if (a.format == CV2_OUT_PCM16) {
        short* out = reinterpret_cast<short*>(a.dst);
        if (full) {
            *reinterpret_cast<s16x4*>(out + tq) = (s16x4){out_pcm16(v[0]), out_pcm16(v[1]), out_pcm16(v[2]), out_pcm16(v[3])};
        } else {
            for (int e = 0; e < 4; e++)
                if (tq + e >= 0 && tq + e < a.n_emit) out[tq + e] = out_pcm16(v[e]);
        }
    } else {
        float* out = reinterpret_cast<float*>(a.dst);
        if (full) {
            *reinterpret_cast<float4*>(out + tq) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int e = 0; e < 4; e++)
                if (tq + e >= 0 && tq + e < a.n_emit) out[tq + e] = v[e];
        }
    }
}

static int out_check(const cv2_out_args& a, int z) {
    CV2_CHECK(a.format == CV2_OUT_F32 || a.format == CV2_OUT_PCM16, "cv2_out_resample: call %d: format %d", z, a.format);
    CV2_CHECK(a.up >= 1 && a.down >= 1 && a.klen >= 1 && a.width >= 0 && a.up <= 4096 && a.down <= 4096 && a.klen <= 4096 && a.width <= 4096,
              "cv2_out_resample: call %d: bad filter shape", z);
    CV2_CHECK(out_span_need(a.up, a.down, a.klen) <= OUT_SPAN, "cv2_out_resample: call %d: up %d, down %d, klen %d need a window of %ld samples, %d fit", z,
              a.up, a.down, a.klen, out_span_need(a.up, a.down, a.klen), OUT_SPAN);
    CV2_CHECK(a.kernel || (a.up == 1 && a.down == 1 && a.klen == 1 && a.width == 0), "cv2_out_resample: call %d: no kernel table", z);
    CV2_CHECK(a.first >= 0 && a.n_tail >= 0 && a.n_avail >= a.first + a.n_tail && a.n_avail <= (1 << 30), "cv2_out_resample: call %d: bad sample counts", z);
    CV2_CHECK(a.n_final == -1 || a.n_final == a.n_avail, "cv2_out_resample: call %d: n_final %d is neither -1 nor n_available %d", z, a.n_final, a.n_avail);
    const int n_new = a.n_avail - a.first - a.n_tail;
    CV2_CHECK((a.n_tail == 0 || a.tail) && (n_new == 0 || a.fresh), "cv2_out_resample: call %d: bad source", z);
    CV2_CHECK(((uintptr_t)a.tail & 3u) == 0 && ((uintptr_t)a.fresh & 3u) == 0 && ((uintptr_t)a.kernel & 3u) == 0, "cv2_out_resample: call %d: misaligned source", z);
    const long o_end = (long)a.o0 + a.n_emit;
    CV2_CHECK(a.o0 >= 0 && a.n_emit >= 0 && o_end * a.down <= (1l << 31) - 1 - (long)a.down * a.up && o_end <= (1 << 30), "cv2_out_resample: call %d: bad output range", z);
    CV2_CHECK(a.n_emit <= a.dst_cap, "cv2_out_resample: call %d: %d samples do not fit a destination of %d", z, a.n_emit, a.dst_cap);
    if (a.n_emit > 0) {
        CV2_CHECK(a.dst && ((uintptr_t)a.dst & (a.format == CV2_OUT_PCM16 ? 1u : 3u)) == 0, "cv2_out_resample: call %d: bad destination", z);
        // every in-range tap of the outputs is one of first .. n_available - 1
        const long lo = (long)(a.o0 / a.up) * a.down - a.width, hi = (long)((o_end - 1) / a.up) * a.down - a.width + a.klen - 1;
        CV2_CHECK((lo > 0 ? lo : 0) >= a.first, "cv2_out_resample: call %d: output %d needs sample %ld, retained from %d on", z, a.o0, lo > 0 ? lo : 0, a.first);
        if (a.n_final < 0)
            CV2_CHECK(hi <= (long)a.n_avail - 1, "cv2_out_resample: call %d: output %ld needs a sample beyond the %d available", z, o_end - 1, a.n_avail);
        else
            CV2_CHECK(o_end <= ((long)a.n_final * a.up + a.down - 1) / a.down, "cv2_out_resample: call %d: output %ld is beyond ceil(%d * %d / %d)", z, o_end - 1,
                      a.n_final, a.up, a.down);
    }
    return 0;
}

static inline int out_blocks(const cv2_out_args& a) { return a.n_emit > 0 ? (a.n_emit + out_shift(a.dst, a.format) + OUT_TO - 1) / OUT_TO : 0; }

extern "C" int cv2_out_resample(const cv2_out_args* a, void* stream) {
    CV2_CHECK(a, "cv2_out_resample: bad argument");
    if (out_check(*a, 0)) return -1;
    if (a->n_emit == 0) return 0;
    hipLaunchKernelGGL(k_out_resample, dim3(out_blocks(*a), 1, 1), dim3(256), 0, (hipStream_t)stream, (const cv2_out_args*)nullptr, *a);
    CV2_LAUNCH_CHECK();
    return 0;
}

extern "C" int cv2_out_resample_batch(const cv2_out_args* args, const cv2_out_args* table_dev, int32_t n, void* stream) {
    CV2_CHECK(args && table_dev && n >= 1 && n <= 65535, "cv2_out_resample_batch: bad argument");
    int blocks = 0;
    for (int z = 0; z < n; z++) {
        if (out_check(args[z], z)) return -1;
        blocks = out_blocks(args[z]) > blocks ? out_blocks(args[z]) : blocks;
    }
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(k_out_resample, dim3(blocks, 1, n), dim3(256), 0, (hipStream_t)stream, table_dev, args[0]);
    CV2_LAUNCH_CHECK();
    return 0;
}
