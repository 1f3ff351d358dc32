// kNN-graph gallery index (engine.nng_knn / nng_optimize / NnGraphIndex / nng_build / nng_search): a
// neighbour table N int32 [n][D] over the rows of a feature store (refine.hip's RefineStore) and a per-query beam search
// that walks it, computing the exact pair distances of the rows it visits.
//
// grl_nng_search, the hot path.  One workgroup of 256 lanes owns one query and runs the whole walk in one launch.  Its LDS
// holds the query row (d * 4 bytes), the sort buffer of P = pow2 >= L + w * D composites (order key << 32 | id; the first
// L are the itopk list C, sorted), the visited table (open addressing, linear probing, H slots of 4 bytes: the id in the
// low 31 bits, the EXPANDED flag of a parent in bit 31, 0xffffffff = empty) and the list of an iteration's new ids.  An
// iteration: wave 0 takes the first w entries of C whose flag is clear and sets it; one lane per (parent, slot) reads N,
// claims the id in the table with an integer atomicCAS and appends a claimed id to the list; the four waves score the
// list, NNG_ROWS rows x 4 (fp32) or 8 (bf16) column chunks in flight per wave, gathered as refine_scan_kernel gathers them
// (wave-uniform ids, 16-byte / 8-byte loads per lane) but loaded raw and widened where they are consumed; lane 0 writes
// the composite behind C and bitonic_lds sorts the buffer.  The pair
// distance is refine.hip's normative order (a private copy: four sequential partials per lane, their join, wave_sum; no
// fma), so it depends on (q, row, d) alone; composites are unique, so the sorted buffer does not depend on the order in
// which the list was filled.  The output distance is the inverse of the order key; a key of zero (-0 and +0 share it)
// is recomputed from the row.  Every branch that leaves the loop tests a value read from LDS behind a barrier.  No
// floating-point atomics, plain vector stores.
//
// grl_nng_detours / grl_nng_merge: the integer passes of the graph optimisation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include "../../include/grl_hip.h"
#include "common.h"
#include "sort_order.h"

#pragma clang fp contract(off)

namespace {

constexpr int NNG_THREADS = 256;
constexpr int NNG_WAVES = NNG_THREADS / 64;
#ifndef GRL_NNG_ROWS
#define GRL_NNG_ROWS 4
#endif
constexpr int NNG_ROWS = GRL_NNG_ROWS;              // store rows in flight per wave
// column chunks of every row in flight: the LDS admits two workgroups per CU at the usual sizes, i.e. two waves per SIMD,
// so the registers are there to keep 4 rows x 4 chunks x 16 bytes (fp32) or 4 x 8 x 8 bytes (bf16) in flight per lane
#ifndef GRL_NNG_TU_F32
#define GRL_NNG_TU_F32 4
#endif
#ifndef GRL_NNG_TU_BF16
#define GRL_NNG_TU_BF16 8
#endif
template <typename T> struct NngTu { static constexpr int value = GRL_NNG_TU_F32; };
template <> struct NngTu<uint16_t> { static constexpr int value = GRL_NNG_TU_BF16; };
constexpr uint32_t NNG_EMPTY = 0xffffffffu, NNG_EXPANDED = 0x80000000u, NNG_ID = 0x7fffffffu;
constexpr uint64_t NNG_PAD = ~0ull;                 // after every real composite (sort_order.h)
constexpr int NNG_CTL = 16;                         // ints: [0] new ids of the iteration, [1] parents, [2..10) their ids

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// a lane's 4 columns of a chunk as they are stored; widened where they are consumed, so that the loads of a batch are
// issued back to back with nothing between them that waits for one
__device__ __forceinline__ f32x4 load_raw(const float* __restrict__ row, int col) {
    return *reinterpret_cast<const f32x4*>(row + col);
}
__device__ __forceinline__ u32x2 load_raw(const uint16_t* __restrict__ row, int col) {
    return *reinterpret_cast<const u32x2*>(row + col);
}
__device__ __forceinline__ f32x4 widen(const f32x4 v) { return v; }
__device__ __forceinline__ f32x4 widen(const u32x2 v) {
    return f32x4{__uint_as_float(v[0] << 16), __uint_as_float(v[0] & 0xffff0000u), __uint_as_float(v[1] << 16),
                 __uint_as_float(v[1] & 0xffff0000u)};
}
template <typename T> struct NngRaw { typedef f32x4 type; };
template <> struct NngRaw<uint16_t> { typedef u32x2 type; };

template <int METRIC>
__device__ __forceinline__ void accumulate(f32x4& a, const f32x4 q, const f32x4 x) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (METRIC == GRL_PQ_COSINE) {
            const float p = q[e] * x[e];
            a[e] = a[e] + p;
        } else {
            const float df = q[e] - x[e];
            const float p = df * df;
            a[e] = a[e] + p;
        }
    }
}

// the pair distances of the staged query to the store rows id[u] >= 0 (wave-uniform), in every lane: steps 1-5 of the
// refinement contract
template <typename T, int METRIC>
__device__ __forceinline__ void score_rows(const float* __restrict__ s_q, const T* __restrict__ store, int64_t lds, int d,
                                           const int (&id)[NNG_ROWS], float (&dist)[NNG_ROWS]) {
    constexpr int NNG_TU = NngTu<T>::value;
    const int lane = threadIdx.x & 63;
    const int full = d >> 8;                                       // chunks in which every lane has its 4 columns
    const int lc = 4 * lane;
    const bool tail = (full << 8) + lc < d;                        // this lane's part of the ragged last chunk (d % 4 == 0)
    const T* row[NNG_ROWS];
    f32x4 acc[NNG_ROWS];
#pragma unroll
    for (int u = 0; u < NNG_ROWS; ++u) {
        row[u] = store + (int64_t)(id[u] >= 0 ? id[u] : 0) * lds;
        acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    typedef typename NngRaw<T>::type raw_t;
    const raw_t zero = raw_t{};                                    // (widens to +0.0f)
    int t = 0;
    for (; t + NNG_TU <= full; t += NNG_TU) {
        raw_t x[NNG_TU][NNG_ROWS];
#pragma unroll
        for (int s = 0; s < NNG_TU; ++s)
#pragma unroll
            for (int u = 0; u < NNG_ROWS; ++u) x[s][u] = id[u] >= 0 ? load_raw(row[u], ((t + s) << 8) + lc) : zero;
#pragma unroll
        for (int s = 0; s < NNG_TU; ++s) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + ((t + s) << 8) + lc);
#pragma unroll
            for (int u = 0; u < NNG_ROWS; ++u) accumulate<METRIC>(acc[u], qv, widen(x[s][u]));
        }
    }
    for (; t < full; ++t) {
        raw_t x[NNG_ROWS];
#pragma unroll
        for (int u = 0; u < NNG_ROWS; ++u) x[u] = id[u] >= 0 ? load_raw(row[u], (t << 8) + lc) : zero;
        const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + (t << 8) + lc);
#pragma unroll
        for (int u = 0; u < NNG_ROWS; ++u) accumulate<METRIC>(acc[u], qv, widen(x[u]));
    }
    if (tail) {                                                    // columns >= d are skipped
        raw_t x[NNG_ROWS];
#pragma unroll
        for (int u = 0; u < NNG_ROWS; ++u) x[u] = id[u] >= 0 ? load_raw(row[u], (full << 8) + lc) : zero;
        const f32x4 qv = *reinterpret_cast<const f32x4*>(s_q + (full << 8) + lc);
#pragma unroll
        for (int u = 0; u < NNG_ROWS; ++u) accumulate<METRIC>(acc[u], qv, widen(x[u]));
    }
#pragma unroll
    for (int u = 0; u < NNG_ROWS; ++u) {
        const float v = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
        const float S = wave_sum(v);
        float r;
        if (METRIC == GRL_PQ_COSINE) r = -S;
        else r = sqrtf(S > 1e-12f ? S : 1e-12f);                   // (a NaN fails the comparison: 1e-12, as refine.hip)
        if (r != r) r = __int_as_float(0x7fc00000);
        dist[u] = r;
    }
}

// composites of the ids list[0 .. cnt) into dst[0 .. cnt): wave v takes the positions v, v + 4, .., NNG_ROWS at a time
template <typename T, int METRIC>
__device__ __forceinline__ void score_list(const float* __restrict__ s_q, const T* __restrict__ store, int64_t lds, int d,
                                           const int* __restrict__ list, int cnt, uint64_t* __restrict__ dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int jb = wave; jb < cnt; jb += NNG_WAVES * NNG_ROWS) {    // (wave-uniform)
        int id[NNG_ROWS];
#pragma unroll
        for (int u = 0; u < NNG_ROWS; ++u) {
            const int j = jb + u * NNG_WAVES;
            id[u] = __builtin_amdgcn_readfirstlane(j < cnt ? list[j] : -1);
        }
        float dist[NNG_ROWS];
        score_rows<T, METRIC>(s_q, store, lds, d, id, dist);
#pragma unroll
        for (int u = 0; u < NNG_ROWS; ++u)
            if (id[u] >= 0 && lane == 0) dst[jb + u * NNG_WAVES] = composite(order_key(dist[u]), id[u]);
    }
}

__device__ __forceinline__ uint32_t nng_hash(uint32_t id, int hbits) { return (id * 2654435761u) >> (32 - hbits); }

// claims `id` in the visited table: true for the one lane that entered it.  The host sizes the table to at least twice
// the ids a call can claim, so a probe ends long before the bound.
__device__ __forceinline__ bool nng_claim(uint32_t* tab, int hbits, uint32_t id) {
    const uint32_t mask = (1u << hbits) - 1u;
    uint32_t h = nng_hash(id, hbits);
    for (uint32_t i = 0; i <= mask; ++i) {
        const uint32_t old = atomicCAS(&tab[h], NNG_EMPTY, id);
        if (old == NNG_EMPTY) return true;
        if ((old & NNG_ID) == id) return false;
        h = (h + 1u) & mask;
    }
    return false;
}

// the slot of an id that is in the table
__device__ __forceinline__ uint32_t nng_find(const uint32_t* tab, int hbits, uint32_t id) {
    const uint32_t mask = (1u << hbits) - 1u;
    uint32_t h = nng_hash(id, hbits);
    for (uint32_t i = 0; i < mask && (tab[h] & NNG_ID) != id; ++i) h = (h + 1u) & mask;
    return h;
}

__device__ __forceinline__ float key_to_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

struct NngArgs {
    const float* q; int64_t ldq;
    const void* store; int64_t lds;
    const int32_t* nbr;
    const int32_t* seeds; int64_t seed_stride;
    float* out; int32_t* oidx; int32_t* stats;
    int n, d, D, L, w, T, S, P, hbits, W;
};

template <typename T, int METRIC>
__global__ __launch_bounds__(NNG_THREADS) void nng_search_kernel(const NngArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nng_smem[];
    float* s_q = reinterpret_cast<float*>(nng_smem);                       // [d]
    uint64_t* s_key = reinterpret_cast<uint64_t*>(nng_smem + (size_t)a.d * 4);     // [P]
    uint32_t* s_tab = reinterpret_cast<uint32_t*>(s_key + a.P);            // [1 << hbits]
    int* s_list = reinterpret_cast<int*>(s_tab + ((size_t)1 << a.hbits));  // [W]
    int* s_ctl = s_list + a.W;                                             // [NNG_CTL]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const int n = a.n, d = a.d, D = a.D, L = a.L, P = a.P, hbits = a.hbits;
    const T* __restrict__ store = reinterpret_cast<const T*>(a.store);

    const float* __restrict__ qrow = a.q + (int64_t)q * a.ldq;
    for (int c = tid * 4; c < d; c += NNG_THREADS * 4)
        *reinterpret_cast<f32x4*>(s_q + c) = *reinterpret_cast<const f32x4*>(qrow + c);
    for (int j = tid; j < (1 << hbits); j += NNG_THREADS) s_tab[j] = NNG_EMPTY;
    for (int j = tid; j < P; j += NNG_THREADS) s_key[j] = NNG_PAD;
    if (tid == 0) s_ctl[0] = 0;
    __syncthreads();

    for (int j = tid; j < a.S; j += NNG_THREADS) {                         // the seeds: C starts as the distinct live ones
        const int s = a.seeds[(int64_t)q * a.seed_stride + j];
        if (s >= 0 && s < n && nng_claim(s_tab, hbits, (uint32_t)s)) s_list[atomicAdd(&s_ctl[0], 1)] = s;
    }
    __syncthreads();
    int cnt = s_ctl[0];
    int visited = cnt, iters = 0;
    score_list<T, METRIC>(s_q, store, a.lds, d, s_list, cnt, s_key);      // (S <= L)
    __syncthreads();
    bitonic_lds(s_key, (float*)nullptr, P);

    for (int it = 0; it < a.T; ++it) {
        if (tid == 0) s_ctl[0] = 0;
        if (wave == 0) {                                                   // the first w entries of C not yet expanded
            int found = 0;
            for (int base = 0; base < L && found < a.w; base += 64) {
                const int j = base + lane;
                const uint64_t key = j < L ? s_key[j] : NNG_PAD;
                bool un = false;
                uint32_t slot = 0;
                if (key != NNG_PAD) {
                    slot = nng_find(s_tab, hbits, (uint32_t)key);
                    un = (s_tab[slot] & NNG_EXPANDED) == 0;
                }
                const unsigned long long m = __ballot(un);
                const int r = found + __popcll(m & ((1ull << lane) - 1ull));
                if (un && r < a.w) {
                    s_ctl[2 + r] = (int)(uint32_t)key;
                    s_tab[slot] |= NNG_EXPANDED;
                }
                found += __popcll(m);
            }
            if (lane == 0) s_ctl[1] = found < a.w ? found : a.w;
        }
        __syncthreads();
        const int npar = s_ctl[1];
        if (npar == 0) break;                                              // (workgroup-uniform: read behind the barrier)
        ++iters;
        if (tid < npar * D) {
            const int p = s_ctl[2 + tid / D];
            const int v = a.nbr[(int64_t)p * D + tid % D];
            if (v >= 0 && v < n && nng_claim(s_tab, hbits, (uint32_t)v)) s_list[atomicAdd(&s_ctl[0], 1)] = v;
        }
        for (int j = L + tid; j < P; j += NNG_THREADS) s_key[j] = NNG_PAD;
        __syncthreads();
        cnt = s_ctl[0];
        visited += cnt;
        if (cnt) {                                                         // (workgroup-uniform)
            score_list<T, METRIC>(s_q, store, a.lds, d, s_list, cnt, s_key + L);
            __syncthreads();
            bitonic_lds(s_key, (float*)nullptr, P);
        }
    }

    float* __restrict__ orow = a.out + (int64_t)q * L;
    int32_t* __restrict__ irow = a.oidx + (int64_t)q * L;
    for (int j = tid; j < L; j += NNG_THREADS) {
        const uint64_t key = s_key[j];
        if (key == NNG_PAD) { orow[j] = INFINITY; irow[j] = -1; continue; }
        irow[j] = (int)(uint32_t)key;
        const uint32_t k = (uint32_t)(key >> 32);
        if (METRIC != GRL_PQ_COSINE || k != 0x80000000u) orow[j] = key_to_float(k);
    }
    if (tid == 0) { a.stats[2 * (int64_t)q] = visited; a.stats[2 * (int64_t)q + 1] = iters; }
    if (METRIC == GRL_PQ_COSINE) {                                         // -0 and +0 share a key: the row decides
        for (int j = wave; j < L; j += NNG_WAVES) {
            const uint64_t key = s_key[j];                                 // (one address per wave)
            if (__builtin_amdgcn_readfirstlane((uint32_t)(key >> 32)) != 0x80000000u) continue;
            int id[NNG_ROWS];
            float dist[NNG_ROWS];
#pragma unroll
            for (int u = 0; u < NNG_ROWS; ++u) id[u] = -1;
            id[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)key);
            score_rows<T, METRIC>(s_q, store, a.lds, d, id, dist);
            if (lane == 0) orow[j] = dist[0];
        }
    }
}

// ---- graph optimisation: detour counts ----
constexpr int DET_THREADS = 256;
constexpr int DET_CHUNK = 64;                                              // pointed-to rows staged at a time

__global__ __launch_bounds__(DET_THREADS) void nng_detours_kernel(const int32_t* __restrict__ knn, int32_t* __restrict__ det,
                                                                  int n, int K) {
    extern __shared__ __attribute__((aligned(16))) int det_smem[];
    int* s_raw = det_smem;                  // [K] row i as given
    int* s_row = s_raw + K;                 // [K] row i, padding as -1
    int* s_det = s_row + K;                 // [K]
    int* s_rows = s_det + K;                // [A][K + 1] the rows t_a of a chunk
    const int tid = threadIdx.x;
    const int A = K < DET_CHUNK ? K : DET_CHUNK, KP = K + 1;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        __syncthreads();
        if (tid < K) s_raw[tid] = knn[(int64_t)i * K + tid];
        __syncthreads();
        if (tid < K) {
            const int v = s_raw[tid];
            bool live = v >= 0 && v < n && v != i;
            for (int b = 0; live && b < tid; ++b) live = s_raw[b] != v;    // a repeat after its first position
            s_row[tid] = live ? v : -1;
            s_det[tid] = live ? 0 : -1;
        }
        for (int a0 = 0; a0 < K; a0 += A) {
            __syncthreads();
            for (int x = tid; x < A * K; x += DET_THREADS) {
                const int al = x / K, r = x - al * K;
                const int ta = a0 + al < K ? s_row[a0 + al] : -1;
                s_rows[al * KP + r] = ta >= 0 ? knn[(int64_t)ta * K + r] : -1;
            }
            __syncthreads();
            for (int x = tid; x < K * A; x += DET_THREADS) {
                const int b = x / A, al = x - b * A, aa = a0 + al;
                if (aa >= b) continue;
                const int tb = s_row[b];
                if (tb < 0 || s_row[aa] < 0) continue;
                bool hit = false;
                for (int r = 0; r < b && !hit; ++r) hit = s_rows[al * KP + r] == tb;
                if (hit) atomicAdd(&s_det[b], 1);
            }
        }
        __syncthreads();
        if (tid < K) det[(int64_t)i * K + tid] = s_det[tid];
    }
}

// ---- graph optimisation: forward / reverse merge, one lane per node ----
constexpr int MRG_THREADS = 64;

__global__ __launch_bounds__(MRG_THREADS) void nng_merge_kernel(const int32_t* __restrict__ fwd, const int64_t* __restrict__ off,
                                                                const int32_t* __restrict__ rev, int32_t* __restrict__ out,
                                                                int n, int D) {
    extern __shared__ __attribute__((aligned(16))) int mrg_smem[];
    int* mine = mrg_smem + threadIdx.x * (D + 1);
    const int half = D >> 1;
    for (int64_t i = (int64_t)blockIdx.x * MRG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MRG_THREADS) {
        const int32_t* f = fwd + i * D;
        int cnt = 0;
        auto has = [&](int v) { for (int c = 0; c < cnt; ++c) if (mine[c] == v) return true; return false; };
        for (int p = 0; p < half; ++p) {
            const int v = f[p];
            if (v >= 0 && !has(v)) mine[cnt++] = v;
        }
        int64_t r = off[i];
        const int64_t end = off[i + 1];
        for (int taken = 0; r < end && taken < half && cnt < D; ++r) {
            const int v = rev[r];
            if (v >= 0 && !has(v)) { mine[cnt++] = v; ++taken; }
        }
        for (int p = half; p < D && cnt < D; ++p) {
            const int v = f[p];
            if (v >= 0 && !has(v)) mine[cnt++] = v;
        }
        for (; r < end && cnt < D; ++r) {
            const int v = rev[r];
            if (v >= 0 && !has(v)) mine[cnt++] = v;
        }
        for (int c = 0; c < D; ++c) out[i * D + c] = c < cnt ? mine[c] : -1;
    }
}

bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// the launch shape of a search call: P, the table's log2 slots, the list ints, the LDS bytes
struct NngShape { int P, hbits, W; int64_t bytes; };

NngShape nng_shape(int64_t n, int d, int D, int L, int w, int64_t T, int S) {
    NngShape s;
    s.P = 8;
    while (s.P < L + w * D) s.P <<= 1;
    int64_t ids = (int64_t)S + T * (int64_t)w * D;                         // what a call can claim: never more than n
    if (ids > n) ids = n;
    s.hbits = 6;
    while (((int64_t)1 << s.hbits) < 2 * ids) ++s.hbits;
    s.W = ((S > w * D ? S : w * D) + 3) & ~3;
    s.bytes = (int64_t)d * 4 + (int64_t)s.P * 8 + ((int64_t)4 << s.hbits) + (int64_t)s.W * 4 + NNG_CTL * 4;
    return s;
}

bool nng_domain(int64_t n, int d, int D, int L, int w, int64_t T, int S) {
    return n >= 0 && n <= INT_MAX && d >= 1 && d <= GRL_REFINE_D_MAX && d % 4 == 0 && D >= 2 && D <= GRL_NNG_D_MAX && D % 2 == 0 &&
           L >= GRL_NNG_L_MIN && L <= GRL_NNG_L_MAX && pow2(L) && w >= 1 && w <= GRL_NNG_W_MAX && w * D <= GRL_NNG_WD_MAX &&
           T >= 1 && T <= INT_MAX && S >= 1 && S <= L;
}

template <typename T>
void nng_launch(int metric, int nq, size_t bytes, hipStream_t st, const NngArgs& a) {
    if (metric == GRL_PQ_COSINE)
        hipLaunchKernelGGL((nng_search_kernel<T, GRL_PQ_COSINE>), dim3((unsigned)nq), dim3(NNG_THREADS), bytes, st, a);
    else
        hipLaunchKernelGGL((nng_search_kernel<T, GRL_PQ_EUCLIDEAN>), dim3((unsigned)nq), dim3(NNG_THREADS), bytes, st, a);
}

}  // namespace

extern "C" int64_t grl_nng_search_lds_bytes(int64_t n, int d, int D, int L, int w, int64_t T, int S) {
    if (!nng_domain(n, d, D, L, w, T, S)) return -1;
    return nng_shape(n, d, D, L, w, T, S).bytes;
}

extern "C" int grl_nng_search(const float* q, int64_t ldq, const void* store, int64_t lds, int store_type, const int32_t* nbr,
                              const int32_t* seeds, int64_t seed_stride, float* out, int32_t* oidx, int32_t* stats, int nq,
                              int64_t n, int d, int D, int L, int w, int T, int S, int metric, void* stream) {
    GRL_REQUIRE(q && store && nbr && seeds && out && oidx && stats, "nng_search: null");
    GRL_REQUIRE(nq >= 0 && nq <= 65535, "nng_search: 0 <= nq <= 65535 queries per call");
    GRL_REQUIRE(nng_domain(n, d, D, L, w, T, S),
                "nng_search: 0 <= n < 2^31, d a multiple of 4 in 1..GRL_REFINE_D_MAX, D even in 2..64, L a power of two in "
                "8..512, 1 <= w <= 8, w * D <= 256, T >= 1 and 1 <= S <= L");
    GRL_REQUIRE(store_type == GRL_REFINE_F32 || store_type == GRL_REFINE_BF16, "nng_search: store_type is not one of GRL_REFINE_*");
    GRL_REQUIRE(metric == GRL_PQ_COSINE || metric == GRL_PQ_EUCLIDEAN, "nng_search: metric is not one of GRL_PQ_*");
    GRL_REQUIRE(ldq >= d && lds >= d && ldq % 4 == 0 && lds % 4 == 0, "nng_search: ldq >= d and lds >= d, both multiples of 4");
    GRL_REQUIRE(seed_stride == 0 || seed_stride >= S, "nng_search: seed_stride must be 0 (shared seeds) or >= S");
    GRL_REQUIRE(aligned16(q) && ((uintptr_t)store & (store_type == GRL_REFINE_F32 ? 15u : 7u)) == 0,
                "nng_search: q and an fp32 store must be 16-byte aligned, a bf16 store 8-byte aligned");
    GRL_REQUIRE((((uintptr_t)nbr | (uintptr_t)seeds | (uintptr_t)out | (uintptr_t)oidx | (uintptr_t)stats) & 3u) == 0,
                "nng_search: nbr, seeds, out, oidx and stats must be 4-byte aligned");
    const NngShape s = nng_shape(n, d, D, L, w, T, S);
    if (s.bytes > GRL_NNG_LDS_MAX)
        return grl_fail(GRL_EINVAL, "nng_search: the query row, the sort buffer and the visited table need %lld bytes of LDS, "
                        "the limit is %d", (long long)s.bytes, GRL_NNG_LDS_MAX);
    if (nq == 0) return GRL_OK;
    NngArgs a;
    a.q = q; a.ldq = ldq; a.store = store; a.lds = lds; a.nbr = nbr; a.seeds = seeds; a.seed_stride = seed_stride;
    a.out = out; a.oidx = oidx; a.stats = stats;
    a.n = (int)n; a.d = d; a.D = D; a.L = L; a.w = w; a.T = T; a.S = S; a.P = s.P; a.hbits = s.hbits; a.W = s.W;
    hipStream_t st = (hipStream_t)stream;
    if (store_type == GRL_REFINE_F32) nng_launch<float>(metric, nq, (size_t)s.bytes, st, a);
    else nng_launch<uint16_t>(metric, nq, (size_t)s.bytes, st, a);
    return grl_check_launch("grl_nng_search");
}

extern "C" int grl_nng_detours(const int32_t* knn, int32_t* det, int64_t n, int K, void* stream) {
    GRL_REQUIRE(knn && det, "nng_detours: null");
    GRL_REQUIRE(n >= 0 && n <= INT_MAX, "nng_detours: 0 <= n < 2^31");
    GRL_REQUIRE(K >= 2 && K <= GRL_NNG_K_MAX, "nng_detours: K must be in 2..GRL_NNG_K_MAX");
    GRL_REQUIRE((((uintptr_t)knn | (uintptr_t)det) & 3u) == 0, "nng_detours: knn and det must be 4-byte aligned");
    if (n == 0) return GRL_OK;
    const int A = K < DET_CHUNK ? K : DET_CHUNK;
    const size_t bytes = (size_t)(3 * K + A * (K + 1)) * sizeof(int);
    const int64_t grid = n < 65536 ? n : 65536;
    hipLaunchKernelGGL(nng_detours_kernel, dim3((unsigned)grid), dim3(DET_THREADS), bytes, (hipStream_t)stream, knn, det, (int)n, K);
    return grl_check_launch("grl_nng_detours");
}

extern "C" int grl_nng_merge(const int32_t* fwd, const int64_t* rev_off, const int32_t* rev, int32_t* out, int64_t n, int D,
                             void* stream) {
    GRL_REQUIRE(fwd && rev_off && rev && out, "nng_merge: null");
    GRL_REQUIRE(n >= 0 && n <= INT_MAX, "nng_merge: 0 <= n < 2^31");
    GRL_REQUIRE(D >= 2 && D <= GRL_NNG_D_MAX && D % 2 == 0, "nng_merge: D must be even in 2..GRL_NNG_D_MAX");
    GRL_REQUIRE((((uintptr_t)fwd | (uintptr_t)rev | (uintptr_t)out) & 3u) == 0 && ((uintptr_t)rev_off & 7u) == 0,
                "nng_merge: fwd, rev and out must be 4-byte aligned, rev_off 8-byte aligned");
    if (n == 0) return GRL_OK;
    const size_t bytes = (size_t)MRG_THREADS * (D + 1) * sizeof(int);
    hipLaunchKernelGGL(nng_merge_kernel, dim3((unsigned)grid_for(n, MRG_THREADS)), dim3(MRG_THREADS), bytes, (hipStream_t)stream,
                       fwd, rev_off, rev, out, (int)n, D);
    return grl_check_launch("grl_nng_merge");
}
