// Generation tail of the layout-token model: the head on one frame's rows, and one sampled decoding step.
//
// vlg_head_frame       final layer-norm + head of the B*N rows m = r*T + t_read only (a rollout uses no other row;
//     vlg_head_last_frame is the t_read = T-1 call: the window is full and slides): one
//     64-lane wavefront per row, the row in registers (d/64 floats per lane, float4 loads when d % 256 == 0), mean and
//     variance by wavefront shuffles exactly as csrc/layernorm.hip, then n_out dot products against the fp32 head weights
//     (each lane reads the columns it holds; a 24 x d weight matrix stays in the vector L1), lane o keeps output o and
//     lanes < n_out store the row of outputs coalesced.  Algorithmic bytes: 4*d per row in, 4*n_out out, 4*n_out*d weights.
// vlg_layout_decode    one block of 64 threads per 64 tokens: the block stages its tokens' rows of out_last in LDS
//     (coalesced; row stride 33 floats = conflict-free per-thread rows), thread i then decodes token i (argmax or the
//     temperature / top-k draw, Philox4x32-10 counter = token and step), writes the generated frame and the last frame of
//     the next window; the T-1 earlier frames of the window are copied by all threads of the grid.  Every store is a plain
//     vector store; no atomics, no state.
// vlg_layout_decode_append  the same step while the history is shorter than the window: the decoding rule is one device
//     function (decode_token) for both; the new frame is written at its position of the window in place, nothing slides.
// vlg_layout_decode_ext / vlg_layout_decode_append_ext  the two steps with a row stride for out_last and, with
//     box_temperature > 0, a box DRAWN from the Gaussian box head's N(mu, (tau sigma)^2) (Box-Muller on the four words of
//     one more Philox call, stream VLG_RNG_BOX_NORMAL): a compile-time parameter of the same kernels and of decode_token, so
//     the instantiation behind the plain entries keeps the rule it always had.
// vlg_layout_decode_samples / vlg_layout_decode_append_samples  the two _ext steps on a batch that holds B / clips SAMPLES of
//     `clips` prompts, sample-major: token (b, n) draws with counter (r0, step, stream, k), r0 = (b % clips)*N + n, k = sample0 +
//     b / clips - one more compile-time parameter of the same kernels (SMP), so every other instantiation keeps its instructions.
// vlg_layout_mix_inputs  scheduled sampling: the inputs of a training step's second pass, per token the truth or the
//     model's own prediction decoded by the same decode_token from the first pass's outputs (end of this file).
// Draws: philox.h (the generator, the word conversions, the seed's key); streams: vlg_rng_stream, include/vlg_hip.h.
#include <type_traits>
#include "common.h"
#include "philox.h"

#define HL_BLOCK 256
#define HL_WAVES (HL_BLOCK / 64)
#define HL_MAX_OUT 32
#define DEC_BLOCK 64
#define DEC_LD (HL_MAX_OUT + 1)

// E = floats per lane; V4: float4 at columns 4*lane + 256*i, else scalars at lane + 64*i (the layouts of layernorm.hip)
template <int E, bool V4>
__device__ __forceinline__ void hl_load(const float* __restrict__ row, int lane, float (&v)[E]) {
    if constexpr (V4) {
#pragma unroll
        for (int i = 0; i < E / 4; ++i) {
            const float4 t = ld4(row + 4 * lane + 256 * i);
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = row[lane + 64 * i];
    }
}

// rows a wave holds per trip (short rows: more bytes in flight, and one pass over the weights serves them all)
#define HL_ROWS(E) ((E) <= 4 ? 2 : 1)

template <int E, bool V4>
__global__ __launch_bounds__(HL_BLOCK) void head_last_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ head_w, const float* __restrict__ head_b, float* __restrict__ out,
    int64_t rows, int T, int t_read, int n_out, float eps) {
    constexpr int d = E * 64, R = HL_ROWS(E);
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * HL_WAVES + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * HL_WAVES;
    float g[E], b[E];
    hl_load<E, V4>(gamma, lane, g);
    hl_load<E, V4>(beta, lane, b);
    const float bias = lane < n_out ? head_b[lane] : 0.f;
    for (int64_t r0 = wave * R; r0 < rows; r0 += nwaves * R) {
        float v[R][E], res[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {                          // a short last group re-reads the last row, stores are guarded
            const int64_t r = r0 + i < rows ? r0 + i : rows - 1;
            hl_load<E, V4>(x + (r * T + t_read) * d, lane, v[i]);
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) s += v[i][j];
            const float mu = wave_sum(s) * (1.0f / d);
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) { const float t = v[i][j] - mu; q += t * t; }
            const float rs = 1.0f / sqrtf(wave_sum(q) * (1.0f / d) + eps);
#pragma unroll
            for (int j = 0; j < E; ++j) v[i][j] = (v[i][j] - mu) * rs * g[j] + b[j];
            res[i] = 0.f;
        }
        for (int o = 0; o < n_out; ++o) {
            float w[E];
            hl_load<E, V4>(head_w + (int64_t)o * d, lane, w);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < E; ++j) a = fmaf(v[i][j], w[j], a);
                a = wave_sum(a);
                if (lane == o) res[i] = a;
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (r0 + i < rows && lane < n_out) out[(r0 + i) * n_out + lane] = res[i] + bias;
    }
}

#define HL_CASE(E) case E: hipLaunchKernelGGL((head_last_kernel<E, (E) % 4 == 0>), grid, block, 0, s, x, gamma, beta, head_w, head_b, \
                                              out_last, rows, T, t_read, n_out, eps); break;

extern "C" int vlg_head_frame(const float* x, const float* gamma, const float* beta, const float* head_w,
                              const float* head_b, float* out_last, int B, int T, int N, int d, int n_out, int t_read,
                              float eps, void* stream) {
    if (B < 1 || T < 1 || N < 1 || d < 64 || d % 64 != 0 || d > 1024 || n_out < 1 || n_out > HL_MAX_OUT) return VLG_ERR_SHAPE;
    if (t_read < 0 || t_read >= T) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(x) || !vlg_aligned16(gamma) || !vlg_aligned16(beta) || !vlg_aligned16(head_w) ||
        !vlg_aligned16(head_b) || !vlg_aligned16(out_last)) return VLG_ERR_ALIGN;
    const int64_t rows = (int64_t)B * N;
    const int E = d / 64, per_block = HL_WAVES * (E <= 4 ? 2 : 1);
    const int64_t nb = (rows + per_block - 1) / per_block;
    const dim3 grid((unsigned)(nb > 4096 ? 4096 : nb)), block(HL_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    switch (E) {
        HL_CASE(1) HL_CASE(2) HL_CASE(3) HL_CASE(4) HL_CASE(5) HL_CASE(6) HL_CASE(7) HL_CASE(8)
        HL_CASE(9) HL_CASE(10) HL_CASE(11) HL_CASE(12) HL_CASE(13) HL_CASE(14) HL_CASE(15) HL_CASE(16)
        default: return VLG_ERR_SHAPE;
    }
    return vlg_last_error();
}

// the frame a sliding rollout reads: the same launch at t_read = T - 1
extern "C" int vlg_head_last_frame(const float* x, const float* gamma, const float* beta, const float* head_w,
                                   const float* head_b, float* out_last, int B, int T, int N, int d, int n_out,
                                   float eps, void* stream) {
    return vlg_head_frame(x, gamma, beta, head_w, head_b, out_last, B, T, N, d, n_out, T - 1, eps, stream);
}

// ---------------------------------------------------------------------------------------------------------- decoding
// The decoding rule, written once for the sliding step, the appending one and the scheduled-sampling mix.  l: token r's [logits | raw box] (the logits
// become the running sums); prev / prev_box: the token's class and box in the newest frame of the history.
// BOX (the Gaussian box head, vlg_layout_decode_ext with box_temperature = tau > 0): l holds [logits | raw mean | raw scale]
// and the box is drawn, box_k = clamp(mu_k + tau sigma_k z_k, 0, 1), z = Box-Muller on the four words of counter
// (r, step, VLG_RNG_BOX_NORMAL, smp); the class draw is untouched.  BOX = false is the rule as it always was, instruction for
// instruction.  smp: the fourth counter word of both draws - the sample index of the _samples entries, 0 from everyone else.
template <bool BOX>
__device__ __forceinline__ void decode_token(float* l, int C, int64_t prev, const float* __restrict__ prev_box, int64_t r, int step,
                                             uint32_t smp, float temperature, int top_k, uint32_t k0, uint32_t k1, int keep_padded,
                                             int64_t& cls, float4& box, float box_tau = 0.f) {
    if (keep_padded && prev >= C) {                        // a padded slot stays padded, box and all
        cls = prev;
        box = ld4(prev_box);
    } else {
        box = make_float4(1.0f / (1.0f + expf(-l[C])), 1.0f / (1.0f + expf(-l[C + 1])),
                          1.0f / (1.0f + expf(-l[C + 2])), 1.0f / (1.0f + expf(-l[C + 3])));
        if constexpr (BOX) {
            uint32_t x[4];
            philox4x32_10((uint32_t)r, (uint32_t)step, VLG_RNG_BOX_NORMAL, smp, k0, k1, x);
            const float rad0 = sqrtf(-2.0f * logf(philox_unit(x[0]))), ang0 = 6.28318530717958648f * philox_unit(x[1]);
            const float rad1 = sqrtf(-2.0f * logf(philox_unit(x[2]))), ang1 = 6.28318530717958648f * philox_unit(x[3]);
            const float z[4] = {rad0 * cosf(ang0), rad0 * sinf(ang0), rad1 * cosf(ang1), rad1 * sinf(ang1)};
            const float mu[4] = {box.x, box.y, box.z, box.w};
            float bx[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float g = 1.0f / (1.0f + expf(-l[C + 4 + k]));
                const float sigma = expf(VLG_BOX_S_MIN + (VLG_BOX_S_MAX - VLG_BOX_S_MIN) * g);
                bx[k] = fminf(fmaxf(mu[k] + box_tau * sigma * z[k], 0.f), 1.f);
            }
            box = make_float4(bx[0], bx[1], bx[2], bx[3]);
        }
        int pick = 0;
        if (temperature == 0.f) {
            float best = l[0];
            for (int c = 1; c < C; ++c)
                if (l[c] > best) { best = l[c]; pick = c; }    // first maximum
        } else {
            uint32_t kept = C >= 32 ? 0xffffffffu : (1u << C) - 1u;
            if (top_k > 0 && top_k < C) {                  // the top_k largest RAW logits, equal values: lower index first
                kept = 0u;
                for (int c = 0; c < C; ++c) {
                    const float lc = l[c];
                    int rank = 0;
                    for (int j = 0; j < C; ++j) rank += (l[j] > lc || (l[j] == lc && j < c)) ? 1 : 0;
                    if (rank < top_k) kept |= 1u << c;
                }
            }
            float m = -INFINITY;
            for (int c = 0; c < C; ++c)
                if ((kept >> c) & 1u) m = fmaxf(m, l[c] / temperature);
            float cum = 0.f;
            for (int c = 0; c < C; ++c) {
                if ((kept >> c) & 1u) cum += expf(l[c] / temperature - m);
                l[c] = cum;
            }
            const uint32_t x0 = philox_word0((uint32_t)r, (uint32_t)step, VLG_RNG_CLASS_DRAW, smp, k0, k1);
            const float u = philox_unit(x0);
            const float thr = u * cum;                     // cum = S
            pick = -1;
            int last_kept = 0;
            for (int c = 0; c < C; ++c)
                if ((kept >> c) & 1u) {
                    last_kept = c;
                    if (pick < 0 && l[c] >= thr) pick = c;
                }
            if (pick < 0) pick = last_kept;
        }
        cls = pick;
    }
}

// stage the first n_out columns of the block's rows of out_last (row stride ld) in LDS; returns the number of tokens of this block
__device__ __forceinline__ int decode_stage(float (*rows)[DEC_LD], const float* __restrict__ out_last, int ld, int64_t BN, int n_out) {
    const int tid = threadIdx.x;
    const int64_t r_first = (int64_t)blockIdx.x * DEC_BLOCK;
    const int here = (int)(BN - r_first < DEC_BLOCK ? BN - r_first : DEC_BLOCK);
    for (int e = tid; e < here * n_out; e += DEC_BLOCK) rows[e / n_out][e % n_out] = out_last[(r_first + e / n_out) * ld + e % n_out];
    __syncthreads();
    return here;
}

// SMP (the _samples entries): the counter's index is the token of the PROMPT, r % (clips*N), and its fourth word the sample
template <bool SMP>
__device__ __forceinline__ void decode_counter(int64_t r, int64_t clips_n, int sample0, int64_t& r0, uint32_t& smp) {
    if constexpr (SMP) {
        const int64_t k = r / clips_n;
        r0 = r - k * clips_n;
        smp = (uint32_t)(sample0 + (int)k);
    } else {
        r0 = r;
        smp = 0u;
    }
}

template <bool BOX, bool SMP>
__global__ __launch_bounds__(DEC_BLOCK) void layout_decode_kernel(
    const float* __restrict__ out_last, int ld, const int64_t* __restrict__ cls_in, const float* __restrict__ box_in,
    int64_t* __restrict__ cls_out, float* __restrict__ box_out, float* __restrict__ valid_out,
    int64_t* __restrict__ gen_cls, float* __restrict__ gen_box, int B, int T, int N, int C, int steps, int step,
    float temperature, int top_k, uint32_t k0, uint32_t k1, int keep_padded, float box_tau, int64_t clips_n, int sample0) {
    __shared__ float rows[DEC_BLOCK][DEC_LD];
    const int tid = threadIdx.x;
    const int64_t BN = (int64_t)B * N, r_first = (int64_t)blockIdx.x * DEC_BLOCK;
    const int here = decode_stage(rows, out_last, ld, BN, C + (BOX ? 8 : 4));
    if (tid < here) {
        const int64_t r = r_first + tid;
        const int b = (int)(r / N), n = (int)(r % N);
        const int64_t last = ((int64_t)b * T + (T - 1)) * N + n;
        int64_t cls, r0;
        uint32_t smp;
        float4 box;
        decode_counter<SMP>(r, clips_n, sample0, r0, smp);
        decode_token<BOX>(rows[tid], C, cls_in[last], box_in + 4 * last, r0, step, smp, temperature, top_k, k0, k1, keep_padded, cls,
                          box, box_tau);
        const int64_t g = ((int64_t)b * steps + step) * N + n;
        gen_cls[g] = cls;
        st4(gen_box + 4 * g, box);
        cls_out[last] = cls;
        st4(box_out + 4 * last, box);
        if (valid_out != nullptr) valid_out[last] = cls < C ? 1.0f : 0.0f;
    }
    // frames 0 .. T-2 of the next window = frames 1 .. T-1 of this one
    const int64_t TN = (int64_t)T * N, keep = TN - N, total = (int64_t)B * TN;
    for (int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + tid; i < total; i += (int64_t)gridDim.x * DEC_BLOCK) {
        if (i % TN >= keep) continue;
        const int64_t c = cls_in[i + N];
        cls_out[i] = c;
        st4(box_out + 4 * i, ld4(box_in + 4 * (i + N)));
        if (valid_out != nullptr) valid_out[i] = c < C ? 1.0f : 0.0f;
    }
}

// what the _ext entries add to the refusals: the row stride, and the box temperature with the columns it needs.  Returns the
// number of columns of a row the kernel reads
// (ext: an _ext entry, whose ld must be a multiple of 4; the plain entries pass ld = n_classes + 4, whatever that is)
static inline int dec_box_columns(int n_classes, int ld, float box_temperature, bool ext) {
    if (ld < n_classes + 4 || (ext && (ld & 3))) return 0;
    if (!(box_temperature >= 0.f) || !(box_temperature <= 3.0e38f)) return 0;           // negative, inf or NaN
    if (box_temperature == 0.f) return n_classes + 4;
    return (ld >= n_classes + 8 && n_classes + 8 <= HL_MAX_OUT) ? n_classes + 8 : 0;
}

// The refusals the four decoding entries share - shape limits, temperature, top_k, steps / step, the box columns, the counter
// range - and, for a call that passes them, what its launch needs: the grid, the seed's key, the columns of a row it reads.
// a batch of samples (the _samples entries): B / clips samples of `clips` prompts, the first of them sample `sample0`; the other
// entries pass none (clips = 0)
struct DecSamples { int clips, sample0; };
struct DecCall {
    int64_t BN;                 // tokens of a frame
    int64_t clips_n;            // tokens of a frame of the prompts: what the counter's index runs over
    int cols;
    dim3 grid;
    PhiloxKey key;
};
static int decode_checks(bool ext, int ld, int B, int T, int N, int n_classes, int steps, int step, float temperature, int top_k,
                         float box_temperature, uint64_t seed, const DecSamples* smp, DecCall& c) {
    if (B < 1 || T < 1 || N < 1 || n_classes < 1 || n_classes + 4 > HL_MAX_OUT) return VLG_ERR_SHAPE;
    if (!(temperature >= 0.f) || !(temperature <= 3.0e38f)) return VLG_ERR_SHAPE;      // negative, inf or NaN
    if (top_k < 0 || top_k > n_classes || steps < 1 || step < 0 || step >= steps) return VLG_ERR_SHAPE;
    c.cols = dec_box_columns(n_classes, ld, box_temperature, ext);
    if (c.cols == 0) return VLG_ERR_SHAPE;
    c.BN = (int64_t)B * N;
    if (!philox_index_fits(c.BN)) return VLG_ERR_SHAPE;                                 // the Philox counter word is the token index
    c.clips_n = c.BN;
    if (smp != nullptr) {                                                               // ... and with samples the last word is the sample
        if (smp->clips < 1 || B % smp->clips != 0 || smp->sample0 < 0) return VLG_ERR_SHAPE;
        if (!philox_index_fits((int64_t)smp->sample0 + B / smp->clips)) return VLG_ERR_SHAPE;
        c.clips_n = (int64_t)smp->clips * N;
    }
    c.grid = dim3((unsigned)((c.BN + DEC_BLOCK - 1) / DEC_BLOCK));
    c.key = philox_key(seed);
    return 0;
}
// box sampling and the sample counter are compile-time parameters of both kernels: the one place where the temperature and
// the entry pick the instantiation
template <typename Launch>
static int decode_launch(float box_temperature, const DecSamples* smp, Launch launch) {
    if (smp != nullptr) {
        if (box_temperature > 0.f) launch(std::true_type(), std::true_type());
        else launch(std::false_type(), std::true_type());
    } else {
        if (box_temperature > 0.f) launch(std::true_type(), std::false_type());
        else launch(std::false_type(), std::false_type());
    }
    return vlg_last_error();
}

static int decode_front(bool ext, const float* out_last, int ld, const int64_t* cls_in, const float* box_in, int64_t* cls_out,
                        float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box, int B, int T, int N,
                        int n_classes, int steps, int step, float temperature, int top_k, float box_temperature,
                        uint64_t seed, int keep_padded, void* stream, const DecSamples* smp = nullptr) {
    DecCall c;
    const int err = decode_checks(ext, ld, B, T, N, n_classes, steps, step, temperature, top_k, box_temperature, seed, smp, c);
    if (err != 0) return err;
    const int64_t BN = c.BN, M = BN * T;
    if (!out_last || !cls_in || !box_in || !cls_out || !box_out || !gen_cls || !gen_box) return VLG_ERR_SHAPE;
    // inputs are only read and outputs only written: any overlap between the two groups is refused
    const void* in_p[3] = {out_last, cls_in, box_in};
    const int64_t in_n[3] = {((BN - 1) * ld + c.cols) * 4, M * 8, M * 16};
    const void* out_p[5] = {cls_out, box_out, valid_out, gen_cls, gen_box};
    const int64_t out_n[5] = {M * 8, M * 16, M * 4, BN * steps * 8, BN * steps * 16};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 5; ++j)
            if (vlg_overlap(in_p[i], in_n[i], out_p[j], out_n[j])) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(out_last) || !vlg_aligned16(box_in) || !vlg_aligned16(box_out) || !vlg_aligned16(gen_box) ||
        !vlg_aligned8(cls_in) || !vlg_aligned8(cls_out) || !vlg_aligned8(gen_cls) || !vlg_aligned4(valid_out)) return VLG_ERR_ALIGN;
    const int sample0 = smp != nullptr ? smp->sample0 : 0;
    return decode_launch(box_temperature, smp, [&](auto box, auto samples) {
        hipLaunchKernelGGL((layout_decode_kernel<decltype(box)::value, decltype(samples)::value>), c.grid, dim3(DEC_BLOCK), 0,
                           (hipStream_t)stream, out_last, ld, cls_in, box_in, cls_out, box_out, valid_out, gen_cls, gen_box, B, T, N,
                           n_classes, steps, step, temperature, top_k, c.key.k0, c.key.k1, keep_padded, box_temperature, c.clips_n,
                           sample0);
    });
}

extern "C" int vlg_layout_decode_ext(const float* out_last, int ld, const int64_t* cls_in, const float* box_in, int64_t* cls_out,
                                     float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box, int B, int T, int N,
                                     int n_classes, int steps, int step, float temperature, int top_k, float box_temperature,
                                     uint64_t seed, int keep_padded, void* stream) {
    return decode_front(true, out_last, ld, cls_in, box_in, cls_out, box_out, valid_out, gen_cls, gen_box, B, T, N, n_classes, steps,
                        step, temperature, top_k, box_temperature, seed, keep_padded, stream);
}

// the same front end on a batch of samples: the counter's index is the prompt's token, its last word the sample
extern "C" int vlg_layout_decode_samples(const float* out_last, int ld, const int64_t* cls_in, const float* box_in, int64_t* cls_out,
                                         float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box, int B, int T, int N,
                                         int n_classes, int steps, int step, float temperature, int top_k, float box_temperature,
                                         uint64_t seed, int keep_padded, int clips, int sample0, void* stream) {
    const DecSamples smp{clips, sample0};
    return decode_front(true, out_last, ld, cls_in, box_in, cls_out, box_out, valid_out, gen_cls, gen_box, B, T, N, n_classes, steps,
                        step, temperature, top_k, box_temperature, seed, keep_padded, stream, &smp);
}

// the ld = n_classes + 4, box_temperature = 0 call of the same front end
extern "C" int vlg_layout_decode(const float* out_last, const int64_t* cls_in, const float* box_in, int64_t* cls_out,
                                 float* box_out, float* valid_out, int64_t* gen_cls, float* gen_box, int B, int T, int N,
                                 int n_classes, int steps, int step, float temperature, int top_k, uint64_t seed,
                                 int keep_padded, void* stream) {
    return decode_front(false, out_last, n_classes + 4, cls_in, box_in, cls_out, box_out, valid_out, gen_cls, gen_box, B, T, N,
                        n_classes, steps, step, temperature, top_k, 0.f, seed, keep_padded, stream);
}

// ---------------------------------------------------------------------------------------- decoding, growing history
// The same step while the history is shorter than the window: nothing slides.  Thread i decodes token i from the newest
// frame pos - 1 and writes frame pos of the window in place, the generated frame and a compact copy of it (the next
// step's embedding input).  64 B per token out; no other element of any buffer is touched.
template <bool BOX, bool SMP>
__global__ __launch_bounds__(DEC_BLOCK) void layout_decode_append_kernel(
    const float* __restrict__ out_last, int ld, int64_t* __restrict__ cls, float* __restrict__ box, float* __restrict__ valid,
    int64_t* __restrict__ gen_cls, float* __restrict__ gen_box, int64_t* __restrict__ frame_cls, float* __restrict__ frame_box,
    int B, int T, int N, int C, int pos, int steps, int step, float temperature, int top_k, uint32_t k0, uint32_t k1,
    int keep_padded, float box_tau, int64_t clips_n, int sample0) {
    __shared__ float rows[DEC_BLOCK][DEC_LD];
    const int tid = threadIdx.x;
    const int64_t BN = (int64_t)B * N, r_first = (int64_t)blockIdx.x * DEC_BLOCK;
    const int here = decode_stage(rows, out_last, ld, BN, C + (BOX ? 8 : 4));
    if (tid >= here) return;
    const int64_t r = r_first + tid;
    const int b = (int)(r / N), n = (int)(r % N);
    const int64_t newest = ((int64_t)b * T + (pos - 1)) * N + n, at = newest + N;
    int64_t c, r0;
    uint32_t smp;
    float4 bx;
    decode_counter<SMP>(r, clips_n, sample0, r0, smp);
    decode_token<BOX>(rows[tid], C, cls[newest], box + 4 * newest, r0, step, smp, temperature, top_k, k0, k1, keep_padded, c, bx,
                      box_tau);
    const int64_t g = ((int64_t)b * steps + step) * N + n;
    gen_cls[g] = c;
    st4(gen_box + 4 * g, bx);
    cls[at] = c;
    st4(box + 4 * at, bx);
    if (valid != nullptr) valid[at] = c < C ? 1.0f : 0.0f;
    frame_cls[r] = c;
    st4(frame_box + 4 * r, bx);
}

static int decode_append_front(bool ext, const float* out_last, int ld, int64_t* cls, float* box, float* valid, int64_t* gen_cls,
                               float* gen_box, int64_t* frame_cls, float* frame_box, int B, int T, int N,
                               int n_classes, int pos, int steps, int step, float temperature, int top_k, float box_temperature,
                               uint64_t seed, int keep_padded, void* stream, const DecSamples* smp = nullptr) {
    DecCall c;
    const int err = decode_checks(ext, ld, B, T, N, n_classes, steps, step, temperature, top_k, box_temperature, seed, smp, c);
    if (err != 0) return err;
    if (pos < 1 || pos >= T) return VLG_ERR_SHAPE;
    const int64_t BN = c.BN, M = BN * T;
    if (!out_last || !cls || !box || !gen_cls || !gen_box || !frame_cls || !frame_box) return VLG_ERR_SHAPE;
    // the window is updated in place (frame pos - 1 read, frame pos written); every other pair of buffers must be disjoint
    const void* p[8] = {out_last, cls, box, valid, gen_cls, gen_box, frame_cls, frame_box};
    const int64_t n[8] = {((BN - 1) * ld + c.cols) * 4, M * 8, M * 16, M * 4, BN * steps * 8, BN * steps * 16, BN * 8, BN * 16};
    for (int i = 0; i < 8; ++i)
        for (int j = i + 1; j < 8; ++j)
            if (vlg_overlap(p[i], n[i], p[j], n[j])) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(out_last) || !vlg_aligned16(box) || !vlg_aligned16(gen_box) || !vlg_aligned16(frame_box) ||
        !vlg_aligned8(cls) || !vlg_aligned8(gen_cls) || !vlg_aligned8(frame_cls) || !vlg_aligned4(valid)) return VLG_ERR_ALIGN;
    const int sample0 = smp != nullptr ? smp->sample0 : 0;
    return decode_launch(box_temperature, smp, [&](auto box_sampled, auto samples) {
        hipLaunchKernelGGL((layout_decode_append_kernel<decltype(box_sampled)::value, decltype(samples)::value>), c.grid,
                           dim3(DEC_BLOCK), 0, (hipStream_t)stream, out_last, ld, cls, box, valid, gen_cls, gen_box, frame_cls, frame_box,
                           B, T, N, n_classes, pos, steps, step, temperature, top_k, c.key.k0, c.key.k1, keep_padded, box_temperature,
                           c.clips_n, sample0);
    });
}

extern "C" int vlg_layout_decode_append_ext(const float* out_last, int ld, int64_t* cls, float* box, float* valid,
                                            int64_t* gen_cls, float* gen_box, int64_t* frame_cls, float* frame_box, int B, int T,
                                            int N, int n_classes, int pos, int steps, int step, float temperature, int top_k,
                                            float box_temperature, uint64_t seed, int keep_padded, void* stream) {
    return decode_append_front(true, out_last, ld, cls, box, valid, gen_cls, gen_box, frame_cls, frame_box, B, T, N, n_classes, pos,
                               steps, step, temperature, top_k, box_temperature, seed, keep_padded, stream);
}

extern "C" int vlg_layout_decode_append_samples(const float* out_last, int ld, int64_t* cls, float* box, float* valid,
                                                int64_t* gen_cls, float* gen_box, int64_t* frame_cls, float* frame_box, int B, int T,
                                                int N, int n_classes, int pos, int steps, int step, float temperature, int top_k,
                                                float box_temperature, uint64_t seed, int keep_padded, int clips, int sample0,
                                                void* stream) {
    const DecSamples smp{clips, sample0};
    return decode_append_front(true, out_last, ld, cls, box, valid, gen_cls, gen_box, frame_cls, frame_box, B, T, N, n_classes, pos,
                               steps, step, temperature, top_k, box_temperature, seed, keep_padded, stream, &smp);
}

// the ld = n_classes + 4, box_temperature = 0 call of the same front end
extern "C" int vlg_layout_decode_append(const float* out_last, int64_t* cls, float* box, float* valid, int64_t* gen_cls,
                                        float* gen_box, int64_t* frame_cls, float* frame_box, int B, int T, int N,
                                        int n_classes, int pos, int steps, int step, float temperature, int top_k,
                                        uint64_t seed, int keep_padded, void* stream) {
    return decode_append_front(false, out_last, n_classes + 4, cls, box, valid, gen_cls, gen_box, frame_cls, frame_box, B, T, N,
                               n_classes, pos, steps, step, temperature, top_k, 0.f, seed, keep_padded, stream);
}

// ------------------------------------------------------------------------------------------------ scheduled sampling
// The inputs of a training step's second pass: per input token the truth or the model's own decoded prediction of it
// (rule: include/vlg_hip.h, "scheduled sampling").  The grid walks `out` in its own row order m = (b*N + n)*T + t, 64 rows
// per block, staged in LDS as decode_stage does (rows with t = T-1 feed nothing and are not loaded).  The thread that holds
// row (r, t), t < T-1, decides input token (b, t+1, n): coin, then decode_token on its row, or the truth; the thread that
// holds row (r, T-1) copies the token of frame 0.  So every token is written by exactly one thread, with plain vector
// stores.  Launch-bound: 4*(C+4) bytes per row read, 2 * 24 bytes per token moved.
__global__ __launch_bounds__(DEC_BLOCK) void layout_mix_inputs_kernel(
    const float* __restrict__ out, int ld, const int64_t* __restrict__ cls, const float* __restrict__ box,
    int64_t* __restrict__ mix_cls, float* __restrict__ mix_box, const int* __restrict__ step_ptr, int64_t M, int T, int N, int C,
    uint32_t thr_max, int ramp_steps, float temperature, int top_k, uint32_t k0, uint32_t k1) {
    __shared__ float rows[DEC_BLOCK][DEC_LD];
    const int tid = threadIdx.x, n_out = C + 4;
    const int64_t m_first = (int64_t)blockIdx.x * DEC_BLOCK;
    const int here = (int)(M - m_first < DEC_BLOCK ? M - m_first : DEC_BLOCK);
    for (int e = tid; e < here * n_out; e += DEC_BLOCK) {
        const int row = e / n_out, col = e - row * n_out;
        const int64_t m = m_first + row;
        if (m % T != T - 1) rows[row][col] = out[m * ld + col];
    }
    __syncthreads();
    if (tid >= here) return;
    const int64_t m = m_first + tid, r = m / T;
    const int t = (int)(m - r * T), b = (int)(r / N), n = (int)(r - (int64_t)b * N);
    const int t_in = t == T - 1 ? 0 : t + 1;                      // the input token this thread writes
    const int64_t i = ((int64_t)b * T + t_in) * N + n;
    int64_t c = cls[i];
    float4 bx = ld4(box + 4 * i);
    if (t_in > 0 && c < C) {
        const int k = *step_ptr;
        const int64_t kk = (int64_t)k + 1;
        const uint32_t thr = ramp_steps == 0 ? thr_max
                                             : (uint32_t)((uint64_t)thr_max * (uint64_t)(kk < ramp_steps ? kk : ramp_steps) / (uint64_t)ramp_steps);
        if (philox_coin(philox_word0((uint32_t)i, (uint32_t)k, VLG_RNG_SCHED_COIN, 0u, k0, k1), thr))
            decode_token<false>(rows[tid], C, c, box + 4 * i, i, k, 0u, temperature, top_k, k0, k1, 0, c, bx);
    }
    mix_cls[i] = c;
    st4(mix_box + 4 * i, bx);
}

extern "C" int vlg_sched_plan(double eps_max, uint32_t* thr_host) {
    if (!(eps_max >= 0.0 && eps_max <= 1.0) || thr_host == nullptr) return VLG_ERR_SHAPE;
    *thr_host = philox_coin_threshold(eps_max);
    return 0;
}

extern "C" int vlg_layout_mix_inputs(const float* out, int ld, const int64_t* cls, const float* box, int64_t* mix_cls,
                                     float* mix_box, const int* step, int B, int T, int N, int n_classes, uint32_t thr_max,
                                     int ramp_steps, float temperature, int top_k, uint64_t seed, void* stream) {
    if (B < 1 || T < 1 || N < 1 || n_classes < 1 || n_classes + 4 > HL_MAX_OUT || ld < n_classes + 4) return VLG_ERR_SHAPE;
    if (!(temperature >= 0.f) || !(temperature <= 3.0e38f)) return VLG_ERR_SHAPE;      // negative, inf or NaN
    if (top_k < 0 || top_k > n_classes || thr_max > (1u << 24) || ramp_steps < 0) return VLG_ERR_SHAPE;
    const int64_t M = (int64_t)B * N * T;
    if (!philox_index_fits(M)) return VLG_ERR_SHAPE;                                    // the Philox counter word is the token index
    if (!out || !cls || !box || !mix_cls || !mix_box || !step) return VLG_ERR_SHAPE;
    // inputs are only read and outputs only written: any overlap between the two groups, or of the two outputs, is refused
    const void* in_p[4] = {out, cls, box, step};
    const int64_t in_n[4] = {((M - 1) * ld + n_classes + 4) * 4, M * 8, M * 16, 4};
    for (int i = 0; i < 4; ++i)
        if (vlg_overlap(in_p[i], in_n[i], mix_cls, M * 8) || vlg_overlap(in_p[i], in_n[i], mix_box, M * 16)) return VLG_ERR_SHAPE;
    if (vlg_overlap(mix_cls, M * 8, mix_box, M * 16)) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(out) || !vlg_aligned16(box) || !vlg_aligned16(mix_box) || !vlg_aligned8(cls) || !vlg_aligned8(mix_cls) ||
        !vlg_aligned4(step)) return VLG_ERR_ALIGN;
    const dim3 grid((unsigned)((M + DEC_BLOCK - 1) / DEC_BLOCK)), block(DEC_BLOCK);
    const PhiloxKey key = philox_key(seed);
    hipLaunchKernelGGL(layout_mix_inputs_kernel, grid, block, 0, (hipStream_t)stream, out, ld, cls, box, mix_cls, mix_box, step, M,
                       T, N, n_classes, thr_max, ramp_steps, temperature, top_k, key.k0, key.k1);
    return vlg_last_error();
}
