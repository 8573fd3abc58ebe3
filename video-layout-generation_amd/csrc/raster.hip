// Rasterised layouts: the slots of a frame drawn into a label map, and the confusion matrix of two label maps.
// Definition: include/vlg_hip.h ("rasterised layouts"); tests/raster_ref.py restates it in fp32 numpy, and the device must
// match it exactly: every quantity is one correctly rounded fp32 operation (written with __f*_rn below, which the compiler
// never contracts), and everything after the edges is integer work.
//
// vlg_layout_rasterize.  A block of 256 threads owns a BAND of rows of one frame (at most RAS_BAND_ROWS, fewer when a
// band of that height holds more than RAS_UNITS thread units per thread: staging and ordering are paid once per band).  It
// first stages the frame's slots into LDS as what the inner loop needs - 16 bytes per slot: the integer pixel ranges [x0, x1) x [y0, y1) the edges cover (four 16-bit fields), the area's
// bits and the label - 256 slots per pass until N (<= 1024: 16 KB, and as much for the ordered copy).  It CULLS while
// staging: only drawn slots whose ranges are not empty and whose rows meet the band enter the list, in slot order (a
// wavefront ballot and a per-wave prefix).
// The block then ORDERS the list by (area, slot index) - a rank sort: entry i counts the entries before it in that order
// (areas are positive floats, compared as unsigned bits; the list position breaks ties) and moves to that place of a
// second list.  A thread owns PX consecutive pixels of a row - 16 for U8 (one 16-byte store), 4 for F32 (one) and I64
// (two) - and walks the ordered list once for all of them: every lane reads the same 16-byte entry (an LDS broadcast),
// turns the slot's pixel range into a bit mask over its PX pixels, and the pixels of the mask that have no winner yet take
// the slot's label: the first slot in the order that covers a pixel is its winner.  A thread stops when all its pixels
// have one, so what a pixel costs is the slots in front of its winner, not the frame's slots.
// The grid is over (frame, band), capped at RAS_MAX_BLOCKS with a grid-stride loop over the rest.
// The integer ranges agree with the definition's comparisons for EVERY edge value, because they are found with those
// comparisons: first_centre() clamps the edge in float (it may be huge or infinite), starts one below its floor and steps
// while `x + 0.5f < edge` holds - two steps always suffice.  x + 0.5f is exact for x <= 16384.
// No block waits for another: no ticket, no spin, no atomics.  Loops are bounded by N or the grid stride, and every barrier
// sits in block-uniform control flow.
//
// vlg_label_confusion.  A thread loads 16 labels of each map with one 16-byte load, turns them into bins truth*L + pred
// (L*L = IGNORED when either label is >= L) and merges runs of equal neighbouring bins in registers before the LDS integer
// atomics: label maps are piecewise constant, so unmerged lanes would pile onto one bin.  When every active lane of a
// wavefront holds one and the same bin for all its 16 pixels - the inside of a large region - one lane adds the
// wavefront's total.  The block's non-zero bins then leave as 64-bit integer atomics (csrc/metrics.hip's counts): the
// result is exact whatever the schedule.  grid.y is the frame index with per_frame; a block's 32-bit bins cannot overflow
// under the entry point's 2^31 bound.
#include "common.h"
#include <float.h>

#define RAS_BLOCK 256
#define RAS_WAVES (RAS_BLOCK / 64)
#define RAS_MAX_SLOTS 1024
#define RAS_MAX_SIDE 16384
#define RAS_BAND_ROWS 32
#define RAS_UNITS 4
#define RAS_MAX_BLOCKS 2048

#define CONF_BLOCK 256
#define CONF_MAX_L 32
#define CONF_MAX_BLOCKS 1024

// the first x in [0, n] whose centre x + 0.5f is >= e (n if there is none); e is never NaN
__device__ __forceinline__ int first_centre(float e, int n) {
    const float c = fminf(fmaxf(e, -1.0f), (float)n + 1.0f);
    int x = max((int)floorf(c) - 1, 0);
    x += ((float)x + 0.5f < e) ? 1 : 0;
    x += ((float)x + 0.5f < e) ? 1 : 0;
    return min(x, n);
}

template <int KIND> struct ras_px { static constexpr int value = KIND == VLG_LABEL_U8 ? 16 : 4; };

template <int KIND>
__device__ __forceinline__ void ras_store(void* labels, int64_t at, const int (&lab)[ras_px<KIND>::value]) {
    if constexpr (KIND == VLG_LABEL_U8) {
        uint4 v;
        v.x = (unsigned)lab[0] | ((unsigned)lab[1] << 8) | ((unsigned)lab[2] << 16) | ((unsigned)lab[3] << 24);
        v.y = (unsigned)lab[4] | ((unsigned)lab[5] << 8) | ((unsigned)lab[6] << 16) | ((unsigned)lab[7] << 24);
        v.z = (unsigned)lab[8] | ((unsigned)lab[9] << 8) | ((unsigned)lab[10] << 16) | ((unsigned)lab[11] << 24);
        v.w = (unsigned)lab[12] | ((unsigned)lab[13] << 8) | ((unsigned)lab[14] << 16) | ((unsigned)lab[15] << 24);
        *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(labels) + at) = v;
    } else if constexpr (KIND == VLG_LABEL_F32) {
        st4(reinterpret_cast<float*>(labels) + at, make_float4((float)lab[0], (float)lab[1], (float)lab[2], (float)lab[3]));
    } else {
        longlong2* p = reinterpret_cast<longlong2*>(reinterpret_cast<int64_t*>(labels) + at);
        p[0] = make_longlong2(lab[0], lab[1]);
        p[1] = make_longlong2(lab[2], lab[3]);
    }
}

template <int KIND>
__global__ __launch_bounds__(RAS_BLOCK) void layout_rasterize_kernel(
    const int64_t* __restrict__ cls, const float* __restrict__ box, const float* __restrict__ valid, void* __restrict__ labels,
    int T_buf, int t0, int T, int N, int n_classes, int H, int W, int what, int background, int band_rows, int bands,
    int64_t items) {
    constexpr int PX = ras_px<KIND>::value;
    __shared__ __attribute__((aligned(16))) int4 list[RAS_MAX_SLOTS];
    __shared__ __attribute__((aligned(16))) int4 sorted[RAS_MAX_SLOTS];
    __shared__ int wcount[RAS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cols = W / PX;
    const float fW = (float)W, fH = (float)H;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t frame = item / bands;
        const int band = (int)(item - frame * bands);
        const int64_t b = frame / T;
        const int t = (int)(frame - b * T);
        const int64_t src0 = (b * T_buf + t0 + t) * N;
        const int ya = band * band_rows, yb = min(H, ya + band_rows);
        // ---- stage and cull: the list keeps slot order
        int count = 0;
        for (int base = 0; base < N; base += RAS_BLOCK) {
            const int n = base + tid;
            bool keep = false;
            int4 e = make_int4(0, 0, 0, 0);
            if (n < N) {
                const int64_t src = src0 + n;
                const int64_t c = cls[src];
                const float4 q = ld4(box + src * 4);
                const float v = valid != nullptr ? valid[src] : 1.0f;
                const bool fin = fabsf(q.x) <= FLT_MAX && fabsf(q.y) <= FLT_MAX && fabsf(q.z) <= FLT_MAX && fabsf(q.w) <= FLT_MAX;
                if (v != 0.f && c >= 0 && c < n_classes && fin && q.z > 0.f && q.w > 0.f) {
                    const float hw = __fmul_rn(0.5f, q.z), hh = __fmul_rn(0.5f, q.w);
                    const int x0 = first_centre(__fmul_rn(__fsub_rn(q.x, hw), fW), W);
                    const int x1 = first_centre(__fmul_rn(__fadd_rn(q.x, hw), fW), W);
                    const int y0 = first_centre(__fmul_rn(__fsub_rn(q.y, hh), fH), H);
                    const int y1 = first_centre(__fmul_rn(__fadd_rn(q.y, hh), fH), H);
                    keep = x0 < x1 && y0 < y1 && y0 < yb && y1 > ya;
                    e = make_int4(x0 | (x1 << 16), y0 | (y1 << 16), (int)__float_as_uint(__fmul_rn(q.z, q.w)),
                                  what == VLG_RASTER_SLOT ? n : (int)c);
                }
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wcount[wave] = __popcll(m);
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < RAS_WAVES; ++w) {
                before += w < wave ? wcount[w] : 0;
                all += wcount[w];
            }
            if (keep) list[count + before + __popcll(m & ((1ull << lane) - 1ull))] = e;
            count += all;
            __syncthreads();                       // the list is complete; wcount is free for the next pass
        }
        // ---- order the list by (area, slot): entry i goes to the number of entries before it in that order (the list is in
        // slot order, so the position breaks ties; list[j].z is one address for all lanes: a broadcast)
        for (int i = tid; i < count; i += RAS_BLOCK) {
            const int4 e = list[i];
            int rank = 0;
            for (int j = 0; j < count; ++j) {
                const unsigned a = (unsigned)list[j].z;
                rank += (a < (unsigned)e.z || (a == (unsigned)e.z && j < i)) ? 1 : 0;
            }
            sorted[rank] = e;
        }
        __syncthreads();
        // ---- draw: PX consecutive pixels of a row per thread; the first slot of the order that covers a pixel is its winner
        const int units = (yb - ya) * cols;
        for (int u = tid; u < units; u += RAS_BLOCK) {
            const int row = u / cols;
            const int y = ya + row, xb = (u - row * cols) * PX;
            constexpr unsigned ALL = (1u << PX) - 1u;
            unsigned done = 0u;
            int lab[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) lab[j] = background;
            for (int s = 0; s < count && done != ALL; ++s) {
                const int4 e = sorted[s];
                const int x0 = e.x & 0xffff, x1 = (int)((unsigned)e.x >> 16), y0 = e.y & 0xffff, y1 = (int)((unsigned)e.y >> 16);
                const int lo = max(x0 - xb, 0), hi = min(x1 - xb, PX);
                if (y >= y0 && y < y1 && lo < hi) {
                    const unsigned fresh = ((1u << hi) - (1u << lo)) & ~done;       // pixels lo .. hi-1 that have no winner yet
                    if (fresh != 0u) {
#pragma unroll
                        for (int j = 0; j < PX; ++j) lab[j] = ((fresh >> j) & 1u) ? e.w : lab[j];
                        done |= fresh;
                    }
                }
            }
            ras_store<KIND>(labels, (frame * H + y) * W + xb, lab);
        }
        __syncthreads();                           // every thread is done with both lists before the next item restages them
    }
}

extern "C" int vlg_layout_rasterize(const int64_t* cls, const float* box, const float* valid, void* labels,
                                    int B, int T_buf, int t0, int T, int N, int n_classes, int H, int W,
                                    int out_kind, int what, int background, void* stream) {
    if (B < 1 || T < 1 || N < 1 || H < 1 || t0 < 0 || (int64_t)t0 + T > T_buf) return VLG_ERR_SHAPE;
    if (N > RAS_MAX_SLOTS || n_classes < 1 || n_classes > 255) return VLG_ERR_SHAPE;
    if (W < 16 || (W & 15) || H > RAS_MAX_SIDE || W > RAS_MAX_SIDE) return VLG_ERR_SHAPE;
    if (background < 0 || background > 255) return VLG_ERR_SHAPE;
    if (out_kind != VLG_LABEL_U8 && out_kind != VLG_LABEL_I64 && out_kind != VLG_LABEL_F32) return VLG_ERR_SHAPE;
    if (what != VLG_RASTER_CLASS && what != VLG_RASTER_SLOT) return VLG_ERR_SHAPE;
    if (what == VLG_RASTER_SLOT && out_kind == VLG_LABEL_U8 && N > 255) return VLG_ERR_SHAPE;
    if (!cls || !box || !labels) return VLG_ERR_SHAPE;
    const int64_t slots = (int64_t)B * T_buf * N, pixels = (int64_t)B * T * H * W;
    const int64_t out_bytes = pixels * (out_kind == VLG_LABEL_U8 ? 1 : out_kind == VLG_LABEL_F32 ? 4 : 8);
    if (vlg_overlap(labels, out_bytes, cls, slots * 8) || vlg_overlap(labels, out_bytes, box, slots * 16) ||
        vlg_overlap(labels, out_bytes, valid, slots * 4)) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(box) || !vlg_aligned16(labels) || !vlg_aligned8(cls) || !vlg_aligned4(valid))
        return VLG_ERR_ALIGN;
    const int cols = W / (out_kind == VLG_LABEL_U8 ? 16 : 4);
    int band_rows = RAS_UNITS * RAS_BLOCK / cols;        // RAS_UNITS thread units per thread: staging is paid once per band
    if (band_rows < 1) band_rows = 1;
    if (band_rows > RAS_BAND_ROWS) band_rows = RAS_BAND_ROWS;
    if (band_rows > H) band_rows = H;
    const int bands = (H + band_rows - 1) / band_rows;
    const int64_t items = (int64_t)B * T * bands;
    const dim3 grid((unsigned)(items < RAS_MAX_BLOCKS ? items : RAS_MAX_BLOCKS)), block(RAS_BLOCK);
    hipStream_t s = (hipStream_t)stream;
#define RAS_LAUNCH(KIND)                                                                                              \
    hipLaunchKernelGGL(layout_rasterize_kernel<KIND>, grid, block, 0, s, cls, box, valid, labels, T_buf, t0, T, N,   \
                       n_classes, H, W, what, background, band_rows, bands, items)
    if (out_kind == VLG_LABEL_U8) RAS_LAUNCH(VLG_LABEL_U8);
    else if (out_kind == VLG_LABEL_F32) RAS_LAUNCH(VLG_LABEL_F32);
    else RAS_LAUNCH(VLG_LABEL_I64);
#undef RAS_LAUNCH
    return vlg_last_error();
}

// ------------------------------------------------------------------------------------------------ confusion
// Segments: with per_frame, block row t reads the B segments (b*T + t)*hw .. + hw; without, the one segment of all B*T*hw
// labels.  vps = 16-label vectors per segment; every index fits 32 bits under the entry point's bound.
__global__ __launch_bounds__(CONF_BLOCK) void label_confusion_kernel(
    const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, unsigned long long* __restrict__ counts,
    int n_seg, int vps, int64_t seg_stride, int64_t row_off, int L) {
    __shared__ int hist[CONF_MAX_L * CONF_MAX_L + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int bins = L * L + 1;
    for (int i = tid; i < bins; i += CONF_BLOCK) hist[i] = 0;
    __syncthreads();
    const int64_t seg0 = (int64_t)blockIdx.y * row_off;
    const int nvec = n_seg * vps;                                     // < 2^27
    for (int v = blockIdx.x * CONF_BLOCK + tid; v < nvec; v += gridDim.x * CONF_BLOCK) {
        const int seg = v / vps;
        const int64_t at = seg0 + seg * seg_stride + (int64_t)(v - seg * vps) * 16;
        const uint4 p4 = *reinterpret_cast<const uint4*>(pred + at);
        const uint4 t4 = *reinterpret_cast<const uint4*>(truth + at);
        const unsigned pw[4] = {p4.x, p4.y, p4.z, p4.w}, tw[4] = {t4.x, t4.y, t4.z, t4.w};
        int cur = 0, run = 0;
        bool flushed = false;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int p = (int)((pw[j >> 2] >> (8 * (j & 3))) & 0xffu), t = (int)((tw[j >> 2] >> (8 * (j & 3))) & 0xffu);
            const int bin = (p < L && t < L) ? t * L + p : L * L;
            if (j == 0) {
                cur = bin;
                run = 1;
            } else if (bin == cur) {
                ++run;
            } else {
                atomicAdd(&hist[cur], run);
                flushed = true;
                cur = bin;
                run = 1;
            }
        }
        // the thread's last run; a wavefront whose active lanes all hold ONE bin adds it once
        const int first = __builtin_amdgcn_readfirstlane(cur);
        const unsigned long long active = __ballot(1);
        if (__ballot(!flushed && cur == first) == active) {
            if (lane == __ffsll((long long)active) - 1) atomicAdd(&hist[first], 16 * __popcll(active));
        } else {
            atomicAdd(&hist[cur], run);
        }
    }
    __syncthreads();
    unsigned long long* row = counts + (int64_t)blockIdx.y * bins;
    for (int i = tid; i < bins; i += CONF_BLOCK)
        if (hist[i] != 0) atomicAdd(row + i, (unsigned long long)hist[i]);
}

extern "C" int vlg_label_confusion(const uint8_t* pred, const uint8_t* truth, int64_t* counts,
                                   int B, int T, int64_t hw, int n_labels, int per_frame, void* stream) {
    if (n_labels < 1 || n_labels > CONF_MAX_L || B < 1 || T < 1 || hw < 16 || (hw & 15)) return VLG_ERR_SHAPE;
    if (hw >= (1LL << 31) || (int64_t)B * T >= (1LL << 31) || (int64_t)B * T * hw >= (1LL << 31)) return VLG_ERR_SHAPE;
    if (!pred || !truth || !counts) return VLG_ERR_SHAPE;
    if (!vlg_aligned16(pred) || !vlg_aligned16(truth) || !vlg_aligned8(counts)) return VLG_ERR_ALIGN;
    const int64_t total = (int64_t)B * T * hw;
    const int rows = per_frame ? T : 1;
    const int n_seg = per_frame ? B : 1;
    const int vps = (int)((per_frame ? hw : total) / 16);
    const int64_t vecs = (int64_t)n_seg * vps;
    int64_t gx = (vecs + CONF_BLOCK - 1) / CONF_BLOCK;
    const int64_t cap = CONF_MAX_BLOCKS / rows > 0 ? CONF_MAX_BLOCKS / rows : 1;
    if (gx > cap) gx = cap;
    if (rows > 65535) return VLG_ERR_SHAPE;                            // grid.y
    hipLaunchKernelGGL(label_confusion_kernel, dim3((unsigned)gx, (unsigned)rows), dim3(CONF_BLOCK), 0, (hipStream_t)stream,
                       pred, truth, reinterpret_cast<unsigned long long*>(counts), n_seg, vps,
                       per_frame ? (int64_t)T * hw : 0, per_frame ? hw : 0, n_labels);
    return vlg_last_error();
}
