// Greedy k-means++ seeding with scikit-learn's arithmetic, driven by scikit-learn's draws (reference:
// wsi_processing/features_clustering.py:10-16, KMeans(n_clusters, random_state=985) -> sklearn _kmeans_plusplus), and the
// centring KMeans.fit does before it.  The host takes the draws from numpy's RandomState (utils/clustering.py) and hands them
// over in a device buffer; everything that depends on the features runs here, K steps enqueued back to back with no host sync:
//
//   dist     squared distances of every row to the step's candidate rows (one pass over X serves all candidates): the candidates'
//            columns are staged in LDS, 16 lanes own a row, sums in f64, clamped at 0 and rounded to f32 (what scikit-learn's
//            float32 path, _euclidean_distances_upcast, returns), element-wise minimum with the closest distances so far, and
//            the workgroup's share of every candidate's potential (f64, rows in order)
//   select   every workgroup adds the shares in one fixed order, takes the first minimum, and copies its slice of the winner's
//            distances into the closest distances; workgroup 0 records the winner's row and potential
//   pick     one workgroup: inclusive f64 scan of the closest distances (scikit-learn's stable_cumsum), rand_t = u_t * potential,
//            candidate_t = #{i : scan_i < rand_t} clipped to N-1 (numpy's left searchsorted + clip)
//
// The first centre is a `dist` + `select` with one candidate (the row the host drew) and no minimum.  No float atomics: the
// result does not depend on scheduling, in either mode (the deterministic mode is not read).
#include "common.h"

#define KPP_KMAX 64
#define KPP_TMAX 6           // 2 + int(log K) candidates per step, K <= 64
#define KPP_DT 2048          // columns of the candidate rows staged in LDS per pass (48 KiB at six candidates)
#define KPP_RB 64            // rows per workgroup of the distance launch
#define KPP_SCAN 1024        // threads of the pick launch
#define KPP_COPY 1024        // rows a workgroup of the select launch copies

static int kpp_trials(int K) {
    int t = 2;                                        // 2 + int(log K) without a libm call on the boundary values
    for (double e = 2.718281828459045; e <= (double)K; e *= 2.718281828459045) ++t;
    return t;
}

template <bool VEC>
__global__ __launch_bounds__(256) void kpp_dist_kernel(const float* __restrict__ X, int N, int d, int T,
                                                        const int* __restrict__ cand, int first,
                                                        const float* __restrict__ closest, float* __restrict__ cand_dist,
                                                        double* __restrict__ part_pot) {
    extern __shared__ __attribute__((aligned(16))) float cs[];        // [T][w] columns [c0, c0 + w) of the candidate rows
    __shared__ double acc[KPP_RB][KPP_TMAX];
    __shared__ float mloc[KPP_RB][KPP_TMAX];
    __shared__ int crow[KPP_TMAX];
    const int t = threadIdx.x, l16 = t & 15, grp = t >> 4;
    if (t < T) crow[t] = first >= 0 ? first : min(max(cand[t], 0), N - 1);
    for (int i = t; i < KPP_RB * KPP_TMAX; i += 256) (&acc[0][0])[i] = 0.0;
    const int r0 = blockIdx.x * KPP_RB;
    for (int c0 = 0; c0 < d; c0 += KPP_DT) {
        const int w = min(KPP_DT, d - c0);
        __syncthreads();                                              // crow / acc written; the previous tile's reads done
        for (int i = t; i < T * w; i += 256) cs[i] = X[(size_t)crow[i / w] * d + c0 + i % w];
        __syncthreads();
        for (int p = 0; p < KPP_RB / 16; ++p) {
            const int rl = p * 16 + grp;
            const float* xr = X + (size_t)min(r0 + rl, N - 1) * d + c0;          // rows past N recompute the last row, unused
            double s[KPP_TMAX];
#pragma unroll
            for (int u = 0; u < KPP_TMAX; ++u) s[u] = 0.0;
            if (VEC) {
                for (int c = 4 * l16; c < w; c += 64) {
                    const f32x4 x = *(const f32x4*)(xr + c);
#pragma unroll
                    for (int u = 0; u < KPP_TMAX; ++u) {
                        if (u < T) {
                            const f32x4 y = *(const f32x4*)(cs + u * w + c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const double df = (double)x[e] - (double)y[e];
                                s[u] = fma(df, df, s[u]);
                            }
                        }
                    }
                }
            } else {
                for (int c = l16; c < w; c += 16) {
                    const double x = (double)xr[c];
#pragma unroll
                    for (int u = 0; u < KPP_TMAX; ++u) {
                        if (u < T) {
                            const double df = x - (double)cs[u * w + c];
                            s[u] = fma(df, df, s[u]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < KPP_TMAX; ++u) {
                if (u < T) {                                          // workgroup-uniform
                    double v = s[u];
                    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
                    if (l16 == 0) acc[rl][u] += v;                    // one writer per (row, candidate): tiles add in column order
                }
            }
        }
    }
    __syncthreads();
    if (t < KPP_RB) {
        const int row = r0 + t;
        for (int u = 0; u < T; ++u) {
            float m = 0.f;
            if (row < N) {
                m = (float)fmax(acc[t][u], 0.0);
                if (closest) m = fminf(m, closest[row]);
                cand_dist[(size_t)u * N + row] = m;
            }
            mloc[t][u] = m;
        }
    }
    __syncthreads();
    if (t < T) {
        double s = 0.0;
        for (int r = 0; r < KPP_RB; ++r) s += (double)mloc[r][t];
        part_pot[(size_t)t * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void kpp_select_kernel(const double* __restrict__ part_pot, int nblk, int T,
                                                          const int* __restrict__ cand, int first,
                                                          const float* __restrict__ cand_dist, int N, float* __restrict__ closest,
                                                          double* __restrict__ pot, int* __restrict__ index_out) {
    __shared__ double red[256];
    __shared__ double pots[KPP_TMAX];
    __shared__ int best_s;
    const int t = threadIdx.x;
    for (int u = 0; u < T; ++u) {                                     // the same order in every workgroup: the same winner
        double s = 0.0;
        for (int j = t; j < nblk; j += 256) s += part_pot[(size_t)u * nblk + j];
        red[t] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) red[t] += red[t + o];
            __syncthreads();
        }
        if (t == 0) pots[u] = red[0];
        __syncthreads();
    }
    if (t == 0) {
        int best = 0;
        for (int u = 1; u < T; ++u)
            if (pots[u] < pots[best]) best = u;                       // first minimum, like numpy's argmin
        best_s = best;
        if (blockIdx.x == 0) {
            *pot = pots[best];
            *index_out = first >= 0 ? first : min(max(cand[best], 0), N - 1);
        }
    }
    __syncthreads();
    const float* src = cand_dist + (size_t)best_s * N;
    const int beg = blockIdx.x * KPP_COPY, end = min(N, beg + KPP_COPY);
    for (int i = beg + t; i < end; i += 256) closest[i] = src[i];
}

__global__ __launch_bounds__(KPP_SCAN) void kpp_pick_kernel(const float* __restrict__ closest, int N, int T,
                                                             const double* __restrict__ pot, const double* __restrict__ uniforms,
                                                             int* __restrict__ cand) {
    __shared__ double sc[2][KPP_SCAN];
    __shared__ int tot[KPP_TMAX];
    const int t = threadIdx.x;
    const int chunk = (N + KPP_SCAN - 1) / KPP_SCAN;
    const int beg = min(N, t * chunk), end = min(N, beg + chunk);
    if (t < KPP_TMAX) tot[t] = 0;
    double s = 0.0;
    for (int i = beg; i < end; ++i) s += (double)closest[i];
    sc[0][t] = s;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < KPP_SCAN; o <<= 1) {                          // inclusive scan of the chunk sums
        sc[cur ^ 1][t] = t >= o ? sc[cur][t] + sc[cur][t - o] : sc[cur][t];
        cur ^= 1;
        __syncthreads();
    }
    double run = t > 0 ? sc[cur][t - 1] : 0.0;
    double rv[KPP_TMAX];
    int cnt[KPP_TMAX];
    const double p = *pot;
#pragma unroll
    for (int u = 0; u < KPP_TMAX; ++u) {
        rv[u] = u < T ? uniforms[u] * p : 0.0;
        cnt[u] = 0;
    }
    for (int i = beg; i < end; ++i) {
        run += (double)closest[i];
#pragma unroll
        for (int u = 0; u < KPP_TMAX; ++u) cnt[u] += (run < rv[u]);
    }
#pragma unroll
    for (int u = 0; u < KPP_TMAX; ++u)
        if (u < T && cnt[u]) atomicAdd(&tot[u], cnt[u]);              // integer counts: the order of arrival changes nothing
    __syncthreads();
    if (t < T) cand[t] = min(tot[t], N - 1);
}

__global__ __launch_bounds__(256) void kpp_gather_kernel(const float* __restrict__ X, int d, const int* __restrict__ indices,
                                                          float* __restrict__ centers) {
    const float* src = X + (size_t)indices[blockIdx.x] * d;
    float* dst = centers + (size_t)blockIdx.x * d;
    for (int c = threadIdx.x; c < d; c += 256) dst[c] = src[c];
}

// workspace, in bytes (every block 16-byte aligned): share of the potentials [T][nblk] f64, potential f64, candidate rows int[8],
// candidate distances [T][N] f32, closest distances [N] f32
struct KppLayout { long part_pot, pot, cand, cand_dist, closest, total; };
static KppLayout kpp_layout(int N, int K) {
    const long T = kpp_trials(K), nblk = (N + KPP_RB - 1) / KPP_RB;
    KppLayout l;
    long o = 0;
    auto take = [&](long bytes) { const long at = o; o += (bytes + 15) & ~15L; return at; };
    l.part_pot = take(T * nblk * 8);
    l.pot = take(8);
    l.cand = take(8 * 4);
    l.cand_dist = take(T * (long)N * 4);
    l.closest = take((long)N * 4);
    l.total = o;
    return l;
}
static bool kpp_ok(int N, int d, int K) { return K >= 1 && K <= KPP_KMAX && N >= K && d >= 1 && (long)N * d < (1L << 40); }

// C-ABI: see include/murcl_amd.h
extern "C" long murcl_kmeans_pp_workspace_bytes(int N, int d, int K) {
    if (!kpp_ok(N, d, K)) return -1;
    return kpp_layout(N, K).total;
}

extern "C" int murcl_kmeans_pp(const float* X, int N, int d, int K, int first, const double* uniforms, int* indices,
                               float* centers, void* workspace, hipStream_t stream) {
    if (!kpp_ok(N, d, K) || first < 0 || first >= N) return -1;
    const KppLayout l = kpp_layout(N, K);
    char* w = (char*)workspace;
    double* part_pot = (double*)(w + l.part_pot);
    double* pot = (double*)(w + l.pot);
    int* cand = (int*)(w + l.cand);
    float* cand_dist = (float*)(w + l.cand_dist);
    float* closest = (float*)(w + l.closest);
    const int T = kpp_trials(K), nblk = (N + KPP_RB - 1) / KPP_RB, ncopy = (N + KPP_COPY - 1) / KPP_COPY;
    const bool vec = d % 4 == 0;
    const int width = d < KPP_DT ? d : KPP_DT;
    auto dist = [&](int t, int row, const float* cl) {
        const int lds = t * width * 4;
        if (vec)
            hipLaunchKernelGGL(kpp_dist_kernel<true>, dim3(nblk), dim3(256), lds, stream, X, N, d, t, (const int*)cand, row, cl,
                               cand_dist, part_pot);
        else
            hipLaunchKernelGGL(kpp_dist_kernel<false>, dim3(nblk), dim3(256), lds, stream, X, N, d, t, (const int*)cand, row, cl,
                               cand_dist, part_pot);
        return MURCL_CHECK_LAUNCH();
    };
    auto select = [&](int t, int row, int c) {
        hipLaunchKernelGGL(kpp_select_kernel, dim3(ncopy), dim3(256), 0, stream, (const double*)part_pot, nblk, t, (const int*)cand,
                           row, (const float*)cand_dist, N, closest, pot, indices + c);
        return MURCL_CHECK_LAUNCH();
    };
    int rc = dist(1, first, nullptr);
    if (rc) return rc;
    rc = select(1, first, 0);
    if (rc) return rc;
    for (int c = 1; c < K; ++c) {
        hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(KPP_SCAN), 0, stream, (const float*)closest, N, T, (const double*)pot,
                           uniforms + (size_t)(c - 1) * T, cand);
        rc = MURCL_CHECK_LAUNCH();
        if (rc) return rc;
        rc = dist(T, -1, closest);
        if (rc) return rc;
        rc = select(T, -1, c);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(kpp_gather_kernel, dim3(K), dim3(256), 0, stream, X, d, (const int*)indices, centers);
    return MURCL_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------- centring (KMeans.fit: X -= X.mean(axis=0))
// column sums in f64: grid (256-column blocks, row parts), a thread adds its column over the part's rows in row order; the parts
// are added in part order, divided by N and rounded to f32; then Xc = X - mean in f32, as numpy subtracts.
#define KPC_PARTS 64

__global__ __launch_bounds__(256) void kpc_colsum_kernel(const float* __restrict__ X, int N, int d, int rows_per_part,
                                                          double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const int beg = blockIdx.y * rows_per_part, end = min(N, beg + rows_per_part);
    double s = 0.0;
    for (int i = beg; i < end; ++i) s += (double)X[(size_t)i * d + c];
    part[(size_t)blockIdx.y * d + c] = s;
}
__global__ __launch_bounds__(256) void kpc_mean_kernel(const double* __restrict__ part, int parts, int N, int d, float* __restrict__ mean) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int p = 0; p < parts; ++p) s += part[(size_t)p * d + c];
    mean[c] = (float)(s / (double)N);
}
__global__ __launch_bounds__(256) void kpc_sub_kernel(const float* __restrict__ X, const float* __restrict__ mean, int N, int d,
                                                       float* __restrict__ Xc) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const float m = mean[c];
    for (int i = blockIdx.y; i < N; i += gridDim.y) Xc[(size_t)i * d + c] = X[(size_t)i * d + c] - m;
}

extern "C" long murcl_kmeans_center_workspace_bytes(int N, int d) {
    if (N < 1 || d < 1) return -1;
    return (long)KPC_PARTS * d * 8;
}

extern "C" int murcl_kmeans_center(const float* X, int N, int d, float* Xc, float* mean, void* workspace, hipStream_t stream) {
    if (N < 1 || d < 1 || (long)N * d >= (1L << 40)) return -1;
    double* part = (double*)workspace;
    const int rows = (N + KPC_PARTS - 1) / KPC_PARTS, parts = (N + rows - 1) / rows, cb = (d + 255) / 256;
    hipLaunchKernelGGL(kpc_colsum_kernel, dim3(cb, parts), dim3(256), 0, stream, X, N, d, rows, part);
    int rc = MURCL_CHECK_LAUNCH();
    if (rc) return rc;
    hipLaunchKernelGGL(kpc_mean_kernel, dim3(cb), dim3(256), 0, stream, (const double*)part, parts, N, d, mean);
    rc = MURCL_CHECK_LAUNCH();
    if (rc) return rc;
    hipLaunchKernelGGL(kpc_sub_kernel, dim3(cb, N < 1024 ? N : 1024), dim3(256), 0, stream, X, (const float*)mean, N, d, Xc);
    return MURCL_CHECK_LAUNCH();
}
