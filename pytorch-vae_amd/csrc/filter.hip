// Validity screen of decoded curves (the reference's prior/filter_curves.py: bond / angle sanity, point and segment
// self-collision, beta strand / sheet heuristics), batched: one workgroup per curve of a padded [B, Lmax, C] batch, then one
// small workgroup that compacts the indices of the kept curves.  Unlike the script, which stops at a curve's first failing
// check, every statistic is computed for every curve and `reason` records the decision (first failing check, script order).
//
// Numerics: the per-curve statistics (bond, angle, rg) are evaluated in fp64 from the fp32 coordinates, two-pass like numpy's
// mean / std.  The O(L^2) pair tests run in fp32 on coordinate DIFFERENCES (p_i - p_j is formed first, segment samples are
// (p0 - q0) + ta * dp - tb * dq), so a compared distance carries ~1e-7 relative error whatever the curve's extent.
#include "common.h"

// mirrors vqh_filter_params_t of include/vqvae_hip.h (tests/test_filter_cpu.py compares the field lists)
#define VQH_FILTER_MAX_LEN 2048
struct vqh_filter_params_t {
    double bond_min_allowed, bond_max_allowed, bond_good_min, bond_good_max, bond_frac_out_max;
    double angle_min_allowed, angle_max_allowed, angle_good_min, angle_good_max, angle_frac_out_max;
    double min_pairwise_dist, seg_min_dist, sheet_min_dist, sheet_max_dist, ss_threshold, min_beta_sheet_fraction;
    int min_length, max_length, neighbor_exclude, seg_neighbor_exclude, seg_num_samples;
    int min_beta_run, min_beta_total, beta_channel, max_isolated_beta_strands, min_strand_len, max_curves;
};

namespace {

constexpr int FT = 256;          // threads per curve
constexpr int FW = FT / 64;      // waves per curve
constexpr int NI = 14, NF = 12;  // output columns

struct SumOp { __device__ double operator()(double a, double b) const { return a + b; } };
struct MinOp { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct MaxOp { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// all FT threads call; v[] holds the block-wide result in every thread afterwards
template <int K, class Op>
__device__ __forceinline__ void block_reduce(double (&v)[K], double* red, Op op) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = op(v[k], __shfl_xor(v[k], o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double r = red[k];
#pragma unroll
        for (int w = 1; w < FW; ++w) r = op(r, red[w * K + k]);
        v[k] = r;
    }
    __syncthreads();
}

constexpr int RED_MAX = 9;       // widest block_reduce below

// pair (i, j), i < j < n, of the row-major upper triangle; step() moves `stride` pairs ahead
struct TriWalk {
    int i, j, n;
    __device__ TriWalk(int n_, int first) : i(0), j(1 + first), n(n_) { wrap(); }
    __device__ void wrap() {
        while (j >= n && i < n - 1) { ++i; j = j - n + i + 1; }
    }
    __device__ bool valid() const { return i < n - 1; }
    __device__ void step(int stride) { j += stride; wrap(); }
};

__global__ __launch_bounds__(FT) void curve_filter_kernel(const float* __restrict__ curves, int Lmax, int C,
                                                          const int* __restrict__ lengths, int ss_logits,
                                                          vqh_filter_params_t P, int* __restrict__ ints,
                                                          float* __restrict__ floats) {
    extern __shared__ float smem[];
    __shared__ double red[FW * RED_MAX];
    float* sx = smem;
    float* sy = sx + Lmax;
    float* sz = sy + Lmax;
    float* sl = sz + Lmax;                                           // bond i -> i+1 length
    unsigned* partner = reinterpret_cast<unsigned*>(sl + Lmax);      // bit i: beta residue i has a sheet partner
    unsigned* beta = partner + (Lmax + 31) / 32;                     // bit i: residue i is beta

    const int b = blockIdx.x, tid = threadIdx.x;
    int n = lengths[b];
    n = n < 0 ? 0 : (n > Lmax ? Lmax : n);
    const int nwords = (Lmax + 31) / 32;
    const bool has_ss = C >= 6 && P.beta_channel >= 0 && P.beta_channel <= 2;
    const float* cur = curves + (size_t)b * Lmax * C;

    for (int w = tid; w < nwords; w += FT) { partner[w] = 0u; beta[w] = 0u; }
    __syncthreads();
    for (int i = tid; i < n; i += FT) {
        const float* p = cur + (size_t)i * C;
        sx[i] = p[0]; sy[i] = p[1]; sz[i] = p[2];
        if (has_ss) {
            bool isb;
            if (ss_logits) {                                         // torch.argmax: first maximum wins
                int am = 0;
                float best = p[3];
                if (p[4] > best) { best = p[4]; am = 1; }
                if (p[5] > best) { am = 2; }
                isb = am == P.beta_channel;
            } else {
                isb = (double)p[3 + P.beta_channel] > P.ss_threshold;
            }
            if (isb) atomicOr(&beta[i >> 5], 1u << (i & 31));
        }
    }
    __syncthreads();

    auto bond = [&](int i) -> double {
        const double dx = (double)sx[i + 1] - (double)sx[i], dy = (double)sy[i + 1] - (double)sy[i],
                     dz = (double)sz[i + 1] - (double)sz[i];
        return sqrt(dx * dx + dy * dy + dz * dz);
    };
    // angle at i+1 in degrees; false when |v1||v2| <= 1e-6 (the reference leaves such angles out)
    auto angle = [&](int i, double& deg) -> bool {
        const double ax = (double)sx[i] - (double)sx[i + 1], ay = (double)sy[i] - (double)sy[i + 1],
                     az = (double)sz[i] - (double)sz[i + 1];
        const double bx = (double)sx[i + 2] - (double)sx[i + 1], by = (double)sy[i + 2] - (double)sy[i + 1],
                     bz = (double)sz[i + 2] - (double)sz[i + 1];
        const double den = sqrt(ax * ax + ay * ay + az * az) * sqrt(bx * bx + by * by + bz * bz);
        if (!(den > 1e-6)) return false;
        double c = (ax * bx + ay * by + az * bz) / den;
        c = fmin(1.0, fmax(-1.0, c));
        deg = acos(c) * (180.0 / 3.14159265358979323846);
        return true;
    };
    auto is_beta = [&](int i) -> bool { return (beta[i >> 5] >> (i & 31)) & 1u; };

    // ---- pass 1: sums, extrema, out-of-range counts
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // bond sum, angle sum, angle num, bond out, angle out, x, y, z, beta total
    double mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int i = tid; i < n; i += FT) {
        s[5] += sx[i]; s[6] += sy[i]; s[7] += sz[i];
        if (is_beta(i)) s[8] += 1.0;
        if (i < n - 1) {
            const double d = bond(i);
            sl[i] = (float)d;
            s[0] += d;
            mn[0] = fmin(mn[0], d); mx[0] = fmax(mx[0], d);
            if (d < P.bond_good_min || d > P.bond_good_max) s[3] += 1.0;
        }
        if (i < n - 2) {
            double a;
            if (angle(i, a)) {
                s[1] += a; s[2] += 1.0;
                mn[1] = fmin(mn[1], a); mx[1] = fmax(mx[1], a);
                if (a < P.angle_good_min || a > P.angle_good_max) s[4] += 1.0;
            }
        }
    }
    block_reduce(s, red, SumOp());
    block_reduce(mn, red, MinOp());
    block_reduce(mx, red, MaxOp());
    const int bond_num = n >= 2 ? n - 1 : 0;
    const int angle_num = (int)s[2];
    const double bond_mean = bond_num ? s[0] / bond_num : 0.0, angle_mean = angle_num ? s[1] / angle_num : 0.0;
    const double cx = n ? s[5] / n : 0.0, cy = n ? s[6] / n : 0.0, cz = n ? s[7] / n : 0.0;
    const int bond_out = (int)s[3], angle_out = (int)s[4], beta_total = (int)s[8];

    // ---- pass 2: squared deviations (numpy's std and the radius of gyration are two-pass)
    double q[3] = {0, 0, 0};
    for (int i = tid; i < n; i += FT) {
        const double dx = sx[i] - cx, dy = sy[i] - cy, dz = sz[i] - cz;
        q[2] += dx * dx + dy * dy + dz * dz;
        if (i < n - 1) { const double d = bond(i) - bond_mean; q[0] += d * d; }
        if (i < n - 2) {
            double a;
            if (angle(i, a)) { a -= angle_mean; q[1] += a * a; }
        }
    }
    block_reduce(q, red, SumOp());

    // ---- pair pass over points: collision count and sheet partners share |p_i - p_j|^2
    double cnt[2] = {0, 0};                      // point pairs (unordered here), segment pairs
    {
        const float pt2 = (float)(P.min_pairwise_dist * P.min_pairwise_dist);
        const float sh_lo = (float)(P.sheet_min_dist * P.sheet_min_dist), sh_hi = (float)(P.sheet_max_dist * P.sheet_max_dist);
        const int ne = P.neighbor_exclude;
        int c = 0;
        for (TriWalk w(n, tid); w.valid(); w.step(FT)) {
            const int i = w.i, j = w.j;
            if (j - i <= ne) continue;
            const float dx = sx[i] - sx[j], dy = sy[i] - sy[j], dz = sz[i] - sz[j];
            const float d2 = dx * dx + dy * dy + dz * dz;
            if (d2 < pt2) ++c;
            if (beta_total && d2 >= sh_lo && d2 <= sh_hi && is_beta(i) && is_beta(j)) {
                atomicOr(&partner[i >> 5], 1u << (i & 31));
                atomicOr(&partner[j >> 5], 1u << (j & 31));
            }
        }
        cnt[0] = c;
    }
    // ---- pair pass over segments: ns x ns sampled distances; a pair whose start points are further apart than the
    // threshold plus both segment lengths cannot have a close sample pair and is skipped
    if (n >= 3) {
        const int nseg = n - 1, ns = P.seg_num_samples, nes = P.seg_neighbor_exclude;
        const float seg2 = (float)(P.seg_min_dist * P.seg_min_dist), thr = (float)P.seg_min_dist;
        const float tstep = ns > 1 ? 1.f / (float)(ns - 1) : 0.f;
        int c = 0;
        for (TriWalk w(nseg, tid); w.valid(); w.step(FT)) {
            const int i = w.i, j = w.j;
            if (j - i <= nes) continue;
            const float ox = sx[i] - sx[j], oy = sy[i] - sy[j], oz = sz[i] - sz[j];
            const float reach = (thr + sl[i] + sl[j]) * 1.001f;
            if (ox * ox + oy * oy + oz * oz > reach * reach) continue;
            const float px = sx[i + 1] - sx[i], py = sy[i + 1] - sy[i], pz = sz[i + 1] - sz[i];
            const float qx = sx[j + 1] - sx[j], qy = sy[j + 1] - sy[j], qz = sz[j + 1] - sz[j];
            bool hit = false;
            for (int a = 0; a < ns; ++a) {
                const float ta = a == ns - 1 && ns > 1 ? 1.f : a * tstep;
                const float ex = ox + ta * px, ey = oy + ta * py, ez = oz + ta * pz;
                for (int bb = 0; bb < ns; ++bb) {
                    const float tb = bb == ns - 1 && ns > 1 ? 1.f : bb * tstep;
                    const float vx = ex - tb * qx, vy = ey - tb * qy, vz = ez - tb * qz;
                    hit |= vx * vx + vy * vy + vz * vz < seg2;
                }
            }
            c += hit;
        }
        cnt[1] = c;
    }
    block_reduce(cnt, red, SumOp());             // its barriers also publish the partner bits

    // ---- beta runs: the thread that owns a run's first residue walks the run
    double bs[3] = {0, 0, 0};                    // strands, strands with a partnered residue, residues with a partner
    double run[1] = {0};
    if (beta_total) {
        for (int i = tid; i < n; i += FT) {
            if (!is_beta(i) || (i > 0 && is_beta(i - 1))) continue;
            int e = i;
            bool sheet = false;
            for (; e < n && is_beta(e); ++e) sheet |= (partner[e >> 5] >> (e & 31)) & 1u;
            const int len = e - i;
            run[0] = fmax(run[0], (double)len);
            if (len >= P.min_strand_len) { bs[0] += 1.0; if (sheet) bs[1] += 1.0; }
        }
        for (int w = tid; w < nwords; w += FT) bs[2] += __popc(partner[w]);
    }
    block_reduce(bs, red, SumOp());
    block_reduce(run, red, MaxOp());

    if (tid != 0) return;
    const int strands = (int)bs[0];
    const int in_sheet = strands ? (int)bs[2] : 0;           // without a strand the reference reports no sheet contacts
    const int strands_sheet = (int)bs[1], strands_iso = strands - strands_sheet, max_run = (int)run[0];
    const double sheet_frac = beta_total ? (double)in_sheet / (double)beta_total : 0.0;
    const double bond_frac = bond_num ? (double)bond_out / bond_num : 0.0;
    const double angle_frac = angle_num ? (double)angle_out / angle_num : 0.0;
    const double bond_min = bond_num ? mn[0] : 0.0, bond_max = bond_num ? mx[0] : 0.0;
    const double angle_min = angle_num ? mn[1] : 0.0, angle_max = angle_num ? mx[1] : 0.0;
    const int self_pairs = 2 * (int)cnt[0], seg_pairs = (int)cnt[1];

    int reason = 0;
    if (n < P.min_length) reason = 1;
    else if (P.max_length > 0 && n > P.max_length) reason = 2;
    else if (bond_num && (bond_min < P.bond_min_allowed || bond_max > P.bond_max_allowed || bond_frac > P.bond_frac_out_max))
        reason = 3;
    else if (angle_num && (angle_min < P.angle_min_allowed || angle_max > P.angle_max_allowed ||
                           angle_frac > P.angle_frac_out_max))
        reason = 4;
    else if (self_pairs > 0) reason = 5;
    else if (seg_pairs > 0) reason = 6;
    else if (has_ss) {
        bool rej = false;
        if (P.min_beta_total > 0 && beta_total > 0 && beta_total < P.min_beta_total) rej = true;
        if (P.min_beta_run > 0 && beta_total > 0 && max_run < P.min_beta_run) rej = true;
        if (P.min_beta_sheet_fraction > 0.0 && beta_total > 0 && sheet_frac < P.min_beta_sheet_fraction) rej = true;
        if (P.max_isolated_beta_strands >= 0 && strands_iso > P.max_isolated_beta_strands) rej = true;
        if (rej) reason = 7;
    }

    int* io = ints + (size_t)b * NI;
    io[0] = n; io[1] = reason; io[2] = bond_num; io[3] = bond_out; io[4] = angle_num; io[5] = angle_out;
    io[6] = self_pairs; io[7] = seg_pairs; io[8] = beta_total; io[9] = max_run; io[10] = in_sheet;
    io[11] = strands; io[12] = strands_sheet; io[13] = strands_iso;
    float* fo = floats + (size_t)b * NF;
    fo[0] = (float)bond_mean; fo[1] = (float)(bond_num ? sqrt(q[0] / bond_num) : 0.0);
    fo[2] = (float)bond_min; fo[3] = (float)bond_max; fo[4] = (float)bond_frac;
    fo[5] = (float)angle_mean; fo[6] = (float)(angle_num ? sqrt(q[1] / angle_num) : 0.0);
    fo[7] = (float)angle_min; fo[8] = (float)angle_max; fo[9] = (float)angle_frac;
    fo[10] = (float)(n ? sqrt(fmax(q[2] / n, 0.0)) : 0.0);
    fo[11] = (float)sheet_frac;
}

// keep_idx[0 .. n_keep) = ascending indices of the curves with reason 0, at most max_curves of them (0 = no cap); the rest
// of keep_idx is -1.  One workgroup: a ballot prefix inside each wave, wave totals through LDS, a running base over chunks.
__global__ __launch_bounds__(FT) void curve_compact_kernel(const int* __restrict__ ints, int B, int max_curves,
                                                           int* __restrict__ keep_idx, int* __restrict__ n_keep) {
    __shared__ int wtot[FW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < B; c0 += FT) {
        const int bi = c0 + tid;
        const bool keep = bi < B && ints[(size_t)bi * NI + 1] == 0;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int off = base, tot = 0;
        for (int w = 0; w < FW; ++w) {
            if (w < wave) off += wtot[w];
            tot += wtot[w];
        }
        const int pos = off + before;
        if (keep && (max_curves <= 0 || pos < max_curves)) keep_idx[pos] = bi;
        base += tot;
        __syncthreads();
    }
    const int nk = max_curves > 0 && base > max_curves ? max_curves : base;
    for (int i = nk + tid; i < B; i += FT) keep_idx[i] = -1;
    if (tid == 0) n_keep[0] = nk;
}

}  // namespace

extern "C" int vqh_curve_filter(const float* curves, int B, int Lmax, int C, const int* lengths, int ss_logits,
                                const vqh_filter_params_t* params, int* ints, float* floats, int* keep_idx, int* n_keep,
                                hipStream_t stream) {
    VQH_CHECK_ARG(B >= 0 && Lmax >= 1 && Lmax <= VQH_FILTER_MAX_LEN && C >= 3, "vqh_curve_filter: need B >= 0, 1 <= Lmax <= 2048, C >= 3");
    VQH_CHECK_ARG(curves && lengths && params && ints && floats && keep_idx && n_keep, "vqh_curve_filter: null pointer");
    VQH_CHECK_ARG(params->seg_num_samples >= 1 && params->seg_num_samples <= 64 && params->neighbor_exclude >= 0 &&
                      params->seg_neighbor_exclude >= 0,
                  "vqh_curve_filter: need 1 <= seg_num_samples <= 64 and neighbour exclusions >= 0");
    if (B > 0) {
        const size_t lds = (size_t)Lmax * 4 * sizeof(float) + 2 * (size_t)((Lmax + 31) / 32) * sizeof(unsigned);
        hipLaunchKernelGGL(curve_filter_kernel, dim3(B), dim3(FT), lds, stream, curves, Lmax, C, lengths, ss_logits, *params,
                           ints, floats);
    }
    hipLaunchKernelGGL(curve_compact_kernel, dim3(1), dim3(FT), 0, stream, ints, B, params->max_curves, keep_idx, n_keep);
    VQH_LAUNCH_CHECK();
    return VQH_OK;
}
