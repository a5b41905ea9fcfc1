// Export of prior-training data (the reference's scripts/extract_code_indices.py and scripts/decode_with_vqvae.py):
//
//   vqh_codes_pack      level-major quantizer ids [Q, B, M] int64 -> per-sample codes [B, M*Q] int32 in the order
//                       t0_l0, t0_l1, ..., t0_l(Q-1), t1_l0, ... (_ensure_batch_first_2d) + the largest id of every row
//   vqh_codes_to_latent the inverse: z_q[b, t, :] = sum over q (ascending, fp32) of E[codes[b, t*Q + q], :] (indices_to_latent);
//                       ids outside 0..K-1 contribute zeros and are counted
//   vqh_latent_geometry compute_latent_geometry_for_sample for a whole padded batch: one workgroup per curve, one wave per
//                       latent token; the curve's valid prefix is staged in LDS (read once from memory, coalesced), segment
//                       sums are wave reductions in fp64 from the fp32 points (two-pass radius, like numpy's), no atomics
//
// None of the three synchronises with the host or allocates, so all of them can be captured into a hipGraph.
#include "common.h"

namespace {

constexpr int ET = 256;              // threads per workgroup
constexpr int EW = ET / 64;          // waves per workgroup
constexpr int GEO_MAX_C = 60;        // G = C + 4 <= 64: one output row per wave-wide store
constexpr int GEO_LDS_BYTES = 64 * 1024;

// one workgroup per sample: reads run along t (contiguous in the level-major source), writes along the row
__global__ __launch_bounds__(ET) void codes_pack_kernel(const long long* __restrict__ idx, int Q, int B, int M,
                                                        int* __restrict__ codes, int* __restrict__ row_max) {
    __shared__ int red[EW];
    const int b = blockIdx.x, tid = threadIdx.x, n = M * Q;
    int mx = INT_MIN;
    for (int j = tid; j < n; j += ET) {
        const int q = j / M, t = j - q * M;
        const int v = (int)idx[((size_t)q * B + b) * M + t];
        codes[(size_t)b * n + (size_t)t * Q + q] = v;
        mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < EW; ++w) mx = red[w] > mx ? red[w] : mx;
        row_max[b] = mx;
    }
}

// VEC = 4: one thread per 16 bytes of an output row (D % 4 == 0, lde % 4 == 0, 16-byte aligned bases); VEC = 1: per float
template <int VEC>
__global__ __launch_bounds__(ET) void codes_to_latent_kernel(const int* __restrict__ codes, long long R, int Q,
                                                             const float* __restrict__ E, int lde, int K, int D,
                                                             float* __restrict__ zq, int* __restrict__ n_bad) {
    const int per_row = D / VEC;
    const long long total = R * per_row;
    for (long long e = (long long)blockIdx.x * ET + threadIdx.x; e < total; e += (long long)gridDim.x * ET) {
        const long long r = e / per_row;
        const int c = (int)(e - r * per_row) * VEC;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        int bad = 0;
        for (int q = 0; q < Q; ++q) {
            const int id = codes[r * Q + q];
            if (id < 0 || id >= K) { ++bad; continue; }
            const float* src = E + (size_t)id * lde + c;
            if constexpr (VEC == 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(src);
                acc[0] += t[0]; acc[1] += t[1]; acc[2] += t[2]; acc[3] += t[3];
            } else {
                acc[0] += src[0];
            }
        }
        float* dst = zq + (size_t)r * D + c;
        if constexpr (VEC == 4) {
            f32x4 t;
            t[0] = acc[0]; t[1] = acc[1]; t[2] = acc[2]; t[3] = acc[3];
            *reinterpret_cast<f32x4*>(dst) = t;
        } else {
            dst[0] = acc[0];
        }
        if (bad && c == 0) atomicAdd(n_bad, bad);      // error path only: each bad id is counted once, by the row's first thread
    }
}

// numpy's np.linspace(0, L, M + 1, dtype=int64)[t]: one fp64 divide, one fp64 multiply, truncation; the end point is L itself
__device__ __forceinline__ int geo_bound(int t, int L, int M) {
    if (t >= M) return L;
    const double step = (double)L / (double)M;
    return (int)(long long)((double)t * step);
}

__global__ __launch_bounds__(ET) void latent_geometry_kernel(const float* __restrict__ x, int Lmax, int C,
                                                             const int* __restrict__ lengths, int M, int Q, int staged,
                                                             float* __restrict__ geo) {
    extern __shared__ float spts[];                    // the curve's valid prefix, [n, C] (when it fits)
    __shared__ float srow[EW][64];                     // one finished row per wave
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = C + 4;
    int n = lengths[b];
    n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
    const float* cur = x + (size_t)b * Lmax * C;
    const float* pts = cur;
    if (staged) {
        for (int i = tid; i < n * C; i += ET) spts[i] = cur[i];
        pts = spts;
    }
    __syncthreads();
    float* out = geo + (size_t)b * M * Q * G;
    for (int t0 = 0; t0 < M; t0 += EW) {               // uniform trip count: the barriers below are workgroup-wide
        const int t = t0 + wave;
        int start = geo_bound(t, n, M), end = geo_bound(t + 1, n, M);
        if (end <= start) end = start + 1 < n ? start + 1 : n;
        const int cnt = end - start;
        if (lane < G) srow[wave][lane] = 0.f;
        if (t < M && cnt > 0) {                        // wave-uniform
            double ctr[3];
            for (int c = 0; c < C; ++c) {              // per-channel mean: centre (0..2), SS mean (3..C-1)
                double s = 0.0;
                for (int i = start + lane; i < end; i += 64) s += (double)pts[(size_t)i * C + c];
                s = wave_sum_d(s) / (double)cnt;
                if (c < 3) ctr[c] = s;
                if (lane == 0) srow[wave][c < 3 ? c : c + 3] = (float)s;
            }
            double r2 = 0.0;
            for (int i = start + lane; i < end; i += 64) {
                const double dx = (double)pts[(size_t)i * C] - ctr[0], dy = (double)pts[(size_t)i * C + 1] - ctr[1],
                             dz = (double)pts[(size_t)i * C + 2] - ctr[2];
                r2 += dx * dx + dy * dy + dz * dz;
            }
            r2 = wave_sum_d(r2);
            if (lane == 0) {
                srow[wave][C + 3] = (float)sqrt(r2 / (double)cnt);
                if (cnt >= 2) {
                    const float* p0 = pts + (size_t)start * C;
                    const float* p1 = pts + (size_t)(end - 1) * C;
                    const double vx = (double)p1[0] - (double)p0[0], vy = (double)p1[1] - (double)p0[1],
                                 vz = (double)p1[2] - (double)p0[2];
                    const double nrm = sqrt(vx * vx + vy * vy + vz * vz) + 1e-8;
                    srow[wave][3] = (float)(vx / nrm);
                    srow[wave][4] = (float)(vy / nrm);
                    srow[wave][5] = (float)(vz / nrm);
                }
            }
        }
        __syncthreads();
        if (t < M) {
            float* dst = out + (size_t)t * Q * G;
            for (int k = lane; k < Q * G; k += 64) dst[k] = srow[wave][k % G];     // the Q repeats of np.repeat: same bits
        }
        __syncthreads();
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int vqh_codes_pack(const long long* idx_level_major, int Q, int B, int M, int* codes, int* row_max,
                              hipStream_t stream) {
    VQH_CHECK_ARG(Q >= 1 && B >= 0 && M >= 1 && (long long)M * Q <= INT_MAX, "vqh_codes_pack: need Q >= 1, B >= 0, M >= 1");
    if (B == 0) return VQH_OK;
    VQH_CHECK_ARG(idx_level_major && codes && row_max, "vqh_codes_pack: null pointer");
    hipLaunchKernelGGL(codes_pack_kernel, dim3(B), dim3(ET), 0, stream, idx_level_major, Q, B, M, codes, row_max);
    VQH_LAUNCH_CHECK();
    return VQH_OK;
}

extern "C" int vqh_codes_to_latent(const int* codes, int B, int M, int Q, const float* E, int lde, int K, int D, float* zq,
                                   int* n_bad, hipStream_t stream) {
    VQH_CHECK_ARG(B >= 0 && M >= 1 && Q >= 1 && K >= 1 && D >= 1 && lde >= D, "vqh_codes_to_latent: bad shape");
    VQH_CHECK_ARG(n_bad, "vqh_codes_to_latent: null pointer");
    hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int), stream);
    if (e != hipSuccess) { vqh_set_error(hipGetErrorString(e)); return VQH_ERR_LAUNCH; }
    if (B == 0) return VQH_OK;
    VQH_CHECK_ARG(codes && E && zq, "vqh_codes_to_latent: null pointer");
    const long long R = (long long)B * M;
    const bool vec = D % 4 == 0 && lde % 4 == 0 && aligned16(E) && aligned16(zq);
    const long long items = R * (vec ? D / 4 : D);
    long long blocks = (items + ET - 1) / ET;
    if (blocks > 65536) blocks = 65536;                // grid-stride beyond that
    if (vec)
        hipLaunchKernelGGL(codes_to_latent_kernel<4>, dim3((unsigned)blocks), dim3(ET), 0, stream, codes, R, Q, E, lde, K, D, zq, n_bad);
    else
        hipLaunchKernelGGL(codes_to_latent_kernel<1>, dim3((unsigned)blocks), dim3(ET), 0, stream, codes, R, Q, E, lde, K, D, zq, n_bad);
    VQH_LAUNCH_CHECK();
    return VQH_OK;
}

extern "C" int vqh_latent_geometry(const float* x, int B, int Lmax, int C, const int* lengths, int M, int Q, float* geo,
                                   hipStream_t stream) {
    VQH_CHECK_ARG(B >= 0 && Lmax >= 1 && C >= 3 && C <= GEO_MAX_C && M >= 1 && Q >= 1,
                  "vqh_latent_geometry: need B >= 0, Lmax >= 1, 3 <= C <= 60, M >= 1, Q >= 1");
    if (B == 0) return VQH_OK;
    VQH_CHECK_ARG(x && lengths && geo, "vqh_latent_geometry: null pointer");
    const size_t bytes = (size_t)Lmax * C * sizeof(float);
    const int staged = bytes <= (size_t)GEO_LDS_BYTES - sizeof(float) * EW * 64;      // longer curves are read from memory
    hipLaunchKernelGGL(latent_geometry_kernel, dim3(B), dim3(ET), staged ? bytes : 0, stream, x, Lmax, C, lengths, M, Q, staged,
                       geo);
    VQH_LAUNCH_CHECK();
    return VQH_OK;
}
