// YOLOv3 detector output -> person boxes in frame pixels (kasf.h, kasf_detect_boxes): what the demo does on the host behind the detector network
//   predict_transform                         demo/lib/yolov3/util.py:34-81
//   write_results (det_hm: persons only)      demo/lib/yolov3/util.py:107-225, bbox_iou demo/lib/yolov3/bbox.py:51-78
//   un-letterbox and clamp                    demo/lib/yolov3/human_detector.py:144-153
// Two launches, no atomics at all, nothing that depends on the order in which lanes or workgroups finish.
// SELECTION (k_detect_select_heads / k_detect_select_rows).  Every candidate owns one 8-byte key slot, one 16-byte box slot and one 4-byte score slot of the
// workspace, at its candidate index (rule 1).  The kernel writes EVERY key slot: 0 for a candidate that fails, otherwise
//   key = order-preserving bits of the objectness << 32 | ~index           (a larger key = a better candidate: higher objectness, then lower index)
// and, for a passing candidate only, its corners at network-input scale and its class score.  Heads form: the tensor is attribute-major, [B][A][5 + C][G * G],
// so lanes map to cells: a wave reads 64 consecutive values of an anchor's objectness plane, and only lanes whose objectness passes go on to the C class planes
// (arg-max on the logits, one sigmoid) and the four box planes -- a frame costs the objectness planes (1 / (5 + C) of the head bytes) plus a few columns.
// Prediction form: one thread per row reads column 4, and the rest of the row only when it passes.
// SORT + NMS + OUTPUT (k_detect_nms).  One workgroup of 1,024 threads per image.  It streams the image's key slots 1,024 at a time and compacts the non-zero
// ones into an LDS buffer of P = 2^k >= max_candidates + 1,024 keys (ballot + prefix counts: no atomics); when the next chunk might not fit, the buffer is
// sorted and cut back to the max_candidates best.  Keys are distinct, so "the max_candidates largest of the set" does not depend on how it was found.  A
// final bitonic sort (of the smallest power of two that holds what is there: 64 keys for a typical frame) gives rule 6's order.  The boxes of the sorted
// candidates are gathered into LDS, greedy NMS runs over them -- one barrier per KEPT box, a suppressed one costs a byte read --, stops at max_boxes survivors,
// and each survivor's row is un-letterboxed and written as it is found.  The library is built with -ffp-contract=off: every expression rounds where the
// reference's torch expression rounds.
#include "kernels.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int NMS_THREADS = 1024;
constexpr int NMS_WAVES = NMS_THREADS / 64;

struct F32 {};
struct F16 {};
struct BF16 {};
template <class E> struct Elem;
template <> struct Elem<F32> {
    using T = float;
    static __device__ inline float up(float v) { return v; }
};
template <> struct Elem<F16> {
    using T = _Float16;
    static __device__ inline float up(_Float16 v) { return (float)v; }
};
template <> struct Elem<BF16> {
    using T = unsigned short;
    static __device__ inline float up(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
};

// fp32 -> 32 bits that order as the values do (-inf lowest, +inf highest); never called with a NaN
__device__ inline unsigned order_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float order_value(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ inline float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ inline bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct Slots {
    unsigned long long* key;   // [B][N]
    float4* box;               // [B][N]  x1, y1, x2, y2 at network-input scale
    float* score;              // [B][N]  class score
};

// rules 3 (done by the caller), 5 and 10, and the slot write of a candidate whose person class won: (x, y, w, h) at network-input scale
__device__ inline void put_candidate(const Slots& s, int64_t slot, int index, float obj, float cls, float x, float y, float w, float h) {
    const float x1 = x - w / 2.0f, y1 = y - h / 2.0f, x2 = x + w / 2.0f, y2 = y + h / 2.0f;
    if (!(finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2))) { s.key[slot] = 0ull; return; }
    s.box[slot] = make_float4(x1, y1, x2, y2);
    s.score[slot] = cls;
    s.key[slot] = ((unsigned long long)order_bits(obj) << 32) | (unsigned)~(unsigned)index;
}

struct HeadArgs {
    const void* src[KASF_DETECT_MAX_SRC];
    int grid[KASF_DETECT_MAX_SRC];                 // G
    int first[KASF_DETECT_MAX_SRC + 1];            // candidate index of the head's first candidate; first[n_src] = N
    float anchor[KASF_DETECT_MAX_SRC][KASF_DETECT_MAX_A][2];   // fp32(anchor / stride), as the reference stores it
    float stride[KASF_DETECT_MAX_SRC];
    int n_src;
};

// grid (ceil(N / SEL_THREADS), B): thread t of image b is "plane position" t: head k, anchor a, cell c with t - first[k] = a * G * G + c
template <class E>
__global__ __launch_bounds__(SEL_THREADS) void k_detect_select_heads(HeadArgs h, int A, int C, float confidence, int class_id, Slots s) {
    using T = typename Elem<E>::T;
    const int N = h.first[h.n_src];
    const int t = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (t >= N) return;
    const int b = blockIdx.y;
    int k = 0;
    while (k + 1 < h.n_src && t >= h.first[k + 1]) ++k;
    const int G = h.grid[k], GG = G * G;
    const int local = t - h.first[k];
    const int a = local / GG, c = local - a * GG;
    const int index = h.first[k] + c * A + a;                                    // rule 1: (cy * G + cx) * A + a behind the earlier heads
    const int64_t slot = (int64_t)b * N + index;
    const T* __restrict__ p = (const T*)h.src[k] + ((int64_t)b * A + a) * (5 + C) * GG + c;   // attribute 0 of this anchor at this cell; attribute i is p[i * GG]
    const float obj = sigmoid_f(Elem<E>::up(p[(int64_t)4 * GG]));
    if (!(obj > confidence)) { s.key[slot] = 0ull; return; }                      // rule 3; a NaN fails it
    // rule 4: the first maximum of the C logits
    float best = Elem<E>::up(p[(int64_t)5 * GG]);
    int arg = 0;
    for (int j = 1; j < C; ++j) {
        const float v = Elem<E>::up(p[(int64_t)(5 + j) * GG]);
        if (v > best) { best = v; arg = j; }
    }
    if (arg != class_id) { s.key[slot] = 0ull; return; }
    // rule 2
    const float st = h.stride[k];
    const int cy = c / G, cx = c - cy * G;
    const float x = (sigmoid_f(Elem<E>::up(p[0])) + (float)cx) * st;
    const float y = (sigmoid_f(Elem<E>::up(p[GG])) + (float)cy) * st;
    const float w = expf(Elem<E>::up(p[(int64_t)2 * GG])) * h.anchor[k][a][0] * st;
    const float hh = expf(Elem<E>::up(p[(int64_t)3 * GG])) * h.anchor[k][a][1] * st;
    put_candidate(s, slot, index, obj, sigmoid_f(best), x, y, w, hh);
}

// grid (ceil(N / SEL_THREADS), B): thread t of image b is row t of prediction [B][N][5 + C]
template <class E>
__global__ __launch_bounds__(SEL_THREADS) void k_detect_select_rows(const typename Elem<E>::T* __restrict__ pred, int N, int C, float confidence,
                                                                    int class_id, Slots s) {
    using T = typename Elem<E>::T;
    const int t = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (t >= N) return;
    const int64_t slot = (int64_t)blockIdx.y * N + t;
    const T* __restrict__ p = pred + slot * (5 + C);
    const float obj = Elem<E>::up(p[4]);
    if (!(obj > confidence)) { s.key[slot] = 0ull; return; }
    float best = Elem<E>::up(p[5]);
    int arg = 0;
    for (int j = 1; j < C; ++j) {
        const float v = Elem<E>::up(p[5 + j]);
        if (v > best) { best = v; arg = j; }
    }
    if (arg != class_id) { s.key[slot] = 0ull; return; }
    put_candidate(s, slot, t, obj, best, Elem<E>::up(p[0]), Elem<E>::up(p[1]), Elem<E>::up(p[2]), Elem<E>::up(p[3]));
}

// descending bitonic sort of keys[0, S), S a power of two, by the whole workgroup; ends with a barrier
__device__ inline void sort_desc(unsigned long long* keys, int S) {
    for (int k = 2; k <= S; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < S; i += NMS_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = keys[i], y = keys[l];
                    const bool down = (i & k) == 0;                              // this run is descending
                    if (down ? x < y : x > y) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}
__device__ inline int pow2_at_least(int n, int floor_) {
    int s = floor_;
    while (s < n) s <<= 1;
    return s;
}

// bbox_iou (bbox.py:51-78) of two corner boxes, every operation a single fp32 operation in the reference's order
__device__ inline float iou_plus_one(const float4 p, const float4 q) {
    const float ix1 = fmaxf(p.x, q.x), iy1 = fmaxf(p.y, q.y), ix2 = fminf(p.z, q.z), iy2 = fminf(p.w, q.w);
    const float inter = fmaxf(ix2 - ix1 + 1.0f, 0.0f) * fmaxf(iy2 - iy1 + 1.0f, 0.0f);
    const float a1 = (p.z - p.x + 1.0f) * (p.w - p.y + 1.0f);
    const float a2 = (q.z - q.x + 1.0f) * (q.w - q.y + 1.0f);
    return inter / (a1 + a2 - inter);
}

// LDS of k_detect_nms: P keys, K boxes, K flags, the wave counts
__host__ __device__ constexpr int64_t nms_lds_bytes(int64_t P, int64_t K) { return P * 8 + K * 16 + ((K + 15) / 16) * 16 + NMS_WAVES * 4; }
constexpr int pow2_ceil_c(int n) { int s = 1; while (s < n) s <<= 1; return s; }
static_assert(nms_lds_bytes(pow2_ceil_c(KASF_DETECT_MAX_CANDIDATES + NMS_THREADS), KASF_DETECT_MAX_CANDIDATES) <= 160 * 1024,
              "k_detect_nms: the largest max_candidates must fit the 160 KiB of LDS of a gfx950 CU");

// grid (B): one workgroup per image.  P = 2^k >= K + NMS_THREADS.
__global__ __launch_bounds__(NMS_THREADS) void k_detect_nms(Slots s, int N, int K, int P, int max_boxes, float nms, float inp,
                                                           const float* __restrict__ frame_wh, float* __restrict__ boxes, int* __restrict__ index,
                                                           int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    float4* box = reinterpret_cast<float4*>(smem + (size_t)P * 8);
    unsigned char* dead = reinterpret_cast<unsigned char*>(smem + (size_t)P * 8 + (size_t)K * 16);
    int* wave_n = reinterpret_cast<int*>(smem + (size_t)P * 8 + (size_t)K * 16 + (size_t)((K + 15) / 16) * 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const unsigned long long* __restrict__ gkey = s.key + (int64_t)b * N;

    for (int i = tid; i < P; i += NMS_THREADS) keys[i] = 0ull;
    __syncthreads();
    int fill = 0, total = 0;                                                     // uniform: keys in the buffer, candidates seen
    for (int base = 0; base < N; base += NMS_THREADS) {
        if (fill + NMS_THREADS > P) {                                            // fill > P - 1,024 >= K: keep the K best
            sort_desc(keys, P);
            for (int i = K + tid; i < P; i += NMS_THREADS) keys[i] = 0ull;
            fill = K;
            __syncthreads();
        }
        const int i = base + tid;
        const unsigned long long k = i < N ? gkey[i] : 0ull;
        const unsigned long long m = __ballot(k != 0ull);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < NMS_WAVES; ++w) {
            const int c = wave_n[w];
            before += w < wave ? c : 0;
            chunk += c;
        }
        if (k != 0ull) keys[fill + before + __popcll(m & ((1ull << lane) - 1ull))] = k;
        fill += chunk;
        total += chunk;
        __syncthreads();
    }
    sort_desc(keys, pow2_at_least(fill, 64));                                    // zeros (free slots) sort last
    const int n = fill < K ? fill : K;

    for (int j = tid; j < n; j += NMS_THREADS) {
        box[j] = s.box[(int64_t)b * N + (int)~(unsigned)keys[j]];
        dead[j] = 0;
    }
    __syncthreads();

    // rule 8 for this image
    const float fw = frame_wh[2 * b], fh = frame_wh[2 * b + 1];
    const float sf = fminf(1.0f / fw * inp, 1.0f / fh * inp);                     // torch evaluates `number / tensor` as reciprocal * number
    const float padx = (inp - sf * fw) / 2.0f, pady = (inp - sf * fh) / 2.0f;
    float* __restrict__ ob = boxes + (int64_t)b * max_boxes * 6;
    int* __restrict__ oi = index + (int64_t)b * max_boxes;

    int kept = 0;
    for (int i = 0; i < n && kept < max_boxes; ++i) {
        if (dead[i]) continue;                                                   // uniform: no write to dead[] since the last barrier
        const float4 p = box[i];
        if (tid == 0) {
            const unsigned long long k = keys[i];
            const int cand = (int)~(unsigned)k;
            float* o = ob + kept * 6;
            o[0] = fminf(fmaxf((p.x - padx) / sf, 0.0f), fw);
            o[1] = fminf(fmaxf((p.y - pady) / sf, 0.0f), fh);
            o[2] = fminf(fmaxf((p.z - padx) / sf, 0.0f), fw);
            o[3] = fminf(fmaxf((p.w - pady) / sf, 0.0f), fh);
            o[4] = order_value((unsigned)(k >> 32));
            o[5] = s.score[(int64_t)b * N + cand];
            oi[kept] = cand;
        }
        ++kept;
        if (kept == max_boxes) break;
        for (int j = i + 1 + tid; j < n; j += NMS_THREADS)
            if (!dead[j] && !(iou_plus_one(p, box[j]) < nms)) dead[j] = 1;       // rule 7: survives iff iou < nms
        __syncthreads();
    }
    for (int r = kept * 6 + tid; r < max_boxes * 6; r += NMS_THREADS) ob[r] = 0.0f;
    for (int r = kept + tid; r < max_boxes; r += NMS_THREADS) oi[r] = -1;
    if (tid == 0) {
        count[2 * b] = kept;
        count[2 * b + 1] = total;
    }
}

Slots carve(void* workspace, int64_t B, int64_t N) {
    char* w = (char*)workspace;
    Slots s;
    s.key = (unsigned long long*)w;
    s.box = (float4*)(w + kasf_detect_round(B * N * 8));
    s.score = (float*)(w + kasf_detect_round(B * N * 8) + kasf_detect_round(B * N * 16));
    return s;
}

}  // namespace

int64_t kasf_detect_ws_bytes(int64_t B, int64_t N) { return kasf_detect_round(B * N * 8) + kasf_detect_round(B * N * 16) + kasf_detect_round(B * N * 4); }

const char* kasf_launch_detect_boxes(hipStream_t st, const void* const* src, int n_src, int form, int dtype, int B, const int* grid, int A, int C,
                                     const float* anchors, int inp_dim, const float* frame_wh, float confidence, float nms, int class_id, int K,
                                     int max_boxes, float* boxes, int* index, int* count, void* workspace) {
    int64_t N = 0;
    HeadArgs h{};
    if (form == KASF_DETECT_FORM_HEADS) {
        h.n_src = n_src;
        for (int k = 0; k < n_src; ++k) {
            const int G = grid[k], stride = inp_dim / G;
            h.src[k] = src[k];
            h.grid[k] = G;
            h.first[k] = (int)N;
            h.stride[k] = (float)stride;
            for (int a = 0; a < A; ++a)
                for (int d = 0; d < 2; ++d) h.anchor[k][a][d] = (float)((double)anchors[(k * A + a) * 2 + d] / (double)stride);   // FloatTensor(a / stride)
            N += (int64_t)G * G * A;
        }
        h.first[n_src] = (int)N;
    } else {
        N = grid[0];
    }
    const Slots s = carve(workspace, B, N);
    const dim3 sgrid((unsigned)((N + SEL_THREADS - 1) / SEL_THREADS), (unsigned)B), sblock(SEL_THREADS);
    if (form == KASF_DETECT_FORM_HEADS) {
        if (dtype == KASF_F32) hipLaunchKernelGGL(k_detect_select_heads<F32>, sgrid, sblock, 0, st, h, A, C, confidence, class_id, s);
        else if (dtype == KASF_F16) hipLaunchKernelGGL(k_detect_select_heads<F16>, sgrid, sblock, 0, st, h, A, C, confidence, class_id, s);
        else hipLaunchKernelGGL(k_detect_select_heads<BF16>, sgrid, sblock, 0, st, h, A, C, confidence, class_id, s);
    } else {
        if (dtype == KASF_F32) hipLaunchKernelGGL(k_detect_select_rows<F32>, sgrid, sblock, 0, st, (const float*)src[0], (int)N, C, confidence, class_id, s);
        else if (dtype == KASF_F16) hipLaunchKernelGGL(k_detect_select_rows<F16>, sgrid, sblock, 0, st, (const _Float16*)src[0], (int)N, C, confidence, class_id, s);
        else hipLaunchKernelGGL(k_detect_select_rows<BF16>, sgrid, sblock, 0, st, (const unsigned short*)src[0], (int)N, C, confidence, class_id, s);
    }
    int P = 1;
    while (P < K + NMS_THREADS) P <<= 1;
    const int64_t lds = nms_lds_bytes(P, K);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_detect_nms), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return "detect_boxes: the device refused the LDS size of the sort + NMS kernel";
    hipLaunchKernelGGL(k_detect_nms, dim3((unsigned)B), dim3(NMS_THREADS), (size_t)lds, st, s, (int)N, K, P, max_boxes, nms, (float)inp_dim, frame_wh, boxes,
                       index, count);
    return nullptr;
}
