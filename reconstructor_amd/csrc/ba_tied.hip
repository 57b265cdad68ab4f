// ba_tied.hip -- the kernels of shared intrinsics (ba_tied.h), for gfx950.
//
// The per-camera reduced system S (lower triangle, n columns, row stride npad) and its right-hand side are built by the solver's own
// kernels; these fold them into the tied system  S' = P' S P,  b' = P' b  that the factorisation reads, expand the solved step, and
// form the few numbers the host judges that must count a tied parameter once.  No float atomics anywhere: every sum has one fixed order,
// so a tied solve is bit-reproducible.  A sum over the members of a group is taken by one wave: lane l adds members l, l + 64, ... in
// ascending order, then the 64 partial sums go through one fixed shuffle tree.
#include "rcn_internal.h"
#include "ba_tied.h"

typedef double f64x2 __attribute__((ext_vector_type(2)));

using ba_tied::Dev;

namespace {

__device__ __forceinline__ double wave_tree(double v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
    return v;      // (lane 0's is the sum)
}
// the first of the four intrinsics columns of camera c (a camera with intrinsics columns has them last)
__device__ __forceinline__ int intr_col0(const Dev &t, int c) { return t.cam_off[c] + t.cam_dim[c] - 4; }

// Rule 1: the Jacobi scale of a group's column, 1 / (1 + sqrt(sum over the members of the raw diagonal)), members in ascending order,
// written into every member's entry of sc.  One thread per column: 4 n_groups threads.
__global__ void k_tied_scale(Dev t, const double *__restrict__ Uraw, double *__restrict__ sc, int jacobi)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 4 * t.n_groups) return;
    const int g = q >> 2, k = q & 3;
    double u = 0.0;
    for (int m = t.grp_off[g]; m < t.grp_off[g + 1]; ++m) { const int c = t.grp_cam[m], s = t.cam_dim[c] - 4 + k; u += Uraw[100 * (size_t)c + 11 * s]; }
    const double v = jacobi ? 1.0 / (1.0 + sqrt(u)) : 1.0;
    for (int m = t.grp_off[g]; m < t.grp_off[g + 1]; ++m) sc[intr_col0(t, t.grp_cam[m]) + k] = v;
}

// Rule 2: the LM diagonal of a group's column is the clamp of the sum, clamp(scale^2 sum raw), kept in dgt and added by the fold; the
// members' own entries of dgc become zero, so the Schur diagonal launch adds no damping of theirs into S.
__global__ void k_tied_diag(Dev t, const double *__restrict__ Uraw, const double *__restrict__ sc, double *__restrict__ dgc, double lo, double hi)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 4 * t.n_groups) return;
    const int g = q >> 2, k = q & 3;
    double u = 0.0;
    for (int m = t.grp_off[g]; m < t.grp_off[g + 1]; ++m) { const int c = t.grp_cam[m], s = t.cam_dim[c] - 4 + k; u += Uraw[100 * (size_t)c + 11 * s]; }
    const double s = sc[intr_col0(t, t.grp_cam[t.grp_off[g]]) + k];
    t.dgt[q] = fmin(fmax(u * s * s, lo), hi);
    for (int m = t.grp_off[g]; m < t.grp_off[g + 1]; ++m) dgc[intr_col0(t, t.grp_cam[m]) + k] = 0.0;
}

// The fold, part 1: the cameras' own columns.  One workgroup per row i of S; row map[i] of S' takes the entries of the columns that are
// some camera's own, in order (own columns keep their order, so the lower triangle stays the lower triangle).  Rows stream with
// 16-byte loads (npad is a multiple of 128: every row is aligned).
__global__ __launch_bounds__(256) void k_tied_fold_own(Dev t, const double *__restrict__ S, const double *__restrict__ rhs)
{
    const int i = blockIdx.x, a = t.map[i];
    if (a >= t.n_own) return;
    const double *row = S + (size_t)i * t.npad;
    double *out = t.S2 + (size_t)a * t.npad_tied;
    for (int j = 2 * threadIdx.x; j <= i; j += 512) {
        const f64x2 v = *reinterpret_cast<const f64x2 *>(row + j);      // (j + 1 <= npad - 1: inside the row)
        const int b0 = t.map[j];
        if (b0 < t.n_own) out[b0] = v[0];
        if (j + 1 <= i) { const int b1 = t.map[j + 1]; if (b1 < t.n_own) out[b1] = v[1]; }
    }
    if (threadIdx.x == 0) t.rhs2[a] = rhs[i];
}

// The fold, part 2: C[i][g][k] = sum over the members c of group g of S(i, column k of c's intrinsics), S read as the symmetric matrix
// its lower triangle stands for.  One wave per (row, group).
__global__ __launch_bounds__(64) void k_tied_fold_rows(Dev t, const double *__restrict__ S)
{
    const int i = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m = t.grp_off[g] + lane; m < t.grp_off[g + 1]; m += 64) {
        const int j0 = intr_col0(t, t.grp_cam[m]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + k;
            acc[k] += j <= i ? S[(size_t)i * t.npad + j] : S[(size_t)j * t.npad + i];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = wave_tree(acc[k]);
    if (lane == 0) {
        double *o = t.C + ((size_t)i * t.n_groups + g) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = acc[k];
    }
}

// The fold, part 3: the groups' rows of S' out of C.  blockIdx.x = g, the row's group; blockIdx.y:
//   g2 <= g      the 4 x 4 block against group g2: the second stage of the corner's sum, over the members of g2 (+ the damping, rule 2)
//   n_groups     the own columns: S'(row, b) = C[src(b)]
//   n_groups + 1 the right-hand side: b'(row) = sum over the members of b
__global__ __launch_bounds__(64) void k_tied_fold_groups(Dev t, const double *__restrict__ rhs, double inv_radius)
{
    const int g = blockIdx.x, y = blockIdx.y, lane = threadIdx.x;
    const int row0 = t.n_own + 4 * g;
    if (y < t.n_groups) {
        const int g2 = y;
        if (g2 > g) return;
        double acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0;
        for (int m = t.grp_off[g2] + lane; m < t.grp_off[g2 + 1]; m += 64) {
            const int j0 = intr_col0(t, t.grp_cam[m]);
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                const double *c = t.C + ((size_t)(j0 + k2) * t.n_groups + g) * 4;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[4 * k + k2] += c[k];
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = wave_tree(acc[e]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) {
                    if (g2 == g && k2 > k) continue;      // (the lower triangle)
                    double v = acc[4 * k + k2];
                    if (g2 == g && k2 == k) v += t.dgt[4 * g + k] * inv_radius;
                    t.S2[(size_t)(row0 + k) * t.npad_tied + t.n_own + 4 * g2 + k2] = v;
                }
        }
    } else if (y == t.n_groups) {
        for (int b = lane; b < t.n_own; b += 64) {
            const double *c = t.C + ((size_t)t.src[t.src_off[b]] * t.n_groups + g) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) t.S2[(size_t)(row0 + k) * t.npad_tied + b] = c[k];
        }
    } else {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int m = t.grp_off[g] + lane; m < t.grp_off[g + 1]; m += 64) {
            const int j0 = intr_col0(t, t.grp_cam[m]);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += rhs[j0 + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = wave_tree(acc[k]);
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) t.rhs2[row0 + k] = acc[k];
    }
}

// Rule 4: delta(i) = delta'(map(i)), into the layout the back-substitution reads.
__global__ void k_tied_expand(Dev t, const double *__restrict__ x, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < t.n) out[i] = x[t.map[i]];
}

// Rule 5, the gradient's max-norm: k_ba_gradmax's, with the gradient of a group's column the sum over its members (ascending) and its
// projection onto the focal bound taken once.  *out zeroed by the caller; max is order-independent, non-negative doubles order like
// their bit patterns.
__global__ __launch_bounds__(256) void k_tied_gradmax(Dev t, const double *__restrict__ gcraw, const double *__restrict__ gpraw, int np3,
                                                      const double *__restrict__ intr, double *out)
{
    __shared__ double sh[4];
    const int t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    auto projected = [&](double g, int col, int c) {
        if (t.mode == 1 && (col == 6 || col == 7)) {
            const double x = intr[6 * c + col - 6];
            double xn = x - g;
            if (xn > t.ub) xn = t.ub;
            g = x - xn;
        }
        return fabs(g);
    };
    double m = 0.0;
    for (int c = t0; c < t.nc; c += stride) {
        const int dc = t.cam_dim[c] - (t.grp[c] >= 0 ? 4 : 0);      // (a member's intrinsics columns: below, once per group)
        for (int k = 0; k < dc; ++k) m = fmax(m, projected(gcraw[10 * (size_t)c + k], t.cols[10 * c + k], c));
    }
    for (int q = t0; q < 4 * t.n_groups; q += stride) {
        const int g = q >> 2, k = q & 3;
        double s = 0.0;
        for (int e = t.grp_off[g]; e < t.grp_off[g + 1]; ++e) { const int c = t.grp_cam[e]; s += gcraw[10 * (size_t)c + t.cam_dim[c] - 4 + k]; }
        const int c0 = t.grp_cam[t.grp_off[g]];
        m = fmax(m, projected(s, t.cols[10 * c0 + t.cam_dim[c0] - 4 + k], c0));
    }
    for (int i = t0; i < np3; i += stride) m = fmax(m, fabs(gpraw[i]));
    for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_down(m, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(m));
    }
}

// Rule 5, the norms of the parameter-tolerance test.  k_ba_plus has summed |dx|^2 and |x|^2 camera by camera: every member of a live
// group has added the group's intrinsics and their step, every held camera its constant intrinsics.  One workgroup takes those terms out
// again and adds each live group once, from its first member -- camera by camera in index order within a thread, then one fixed tree.
// scal[3] = |dx|^2, scal[4] = |x|^2 (as k_ba_plus left them; g.delta needs nothing: the members' terms add up to the group's).
__global__ __launch_bounds__(256) void k_tied_norms(Dev t, const double *__restrict__ intr, const double *__restrict__ intr2, double *scal)
{
    __shared__ double sh[2][4];
    double dn = 0.0, xn = 0.0;
    for (int c = threadIdx.x; c < t.nc; c += 256) {
        const int g = t.grp[c];
        if (g == ba_tied::OWN) continue;
        // what k_ba_plus counted for this camera (its `used && mode == 1 && dc > 0`, and the step of all six intrinsics)
        const bool used = t.cam_obs_off[c + 1] > t.cam_obs_off[c], counted = used && t.mode == 1 && t.cam_dim[c] > 0;
        double x2 = 0.0, d2 = 0.0;
        for (int k = 0; k < 6; ++k) { const double x = intr[6 * c + k], dd = intr2[6 * c + k] - x; x2 += x * x; d2 += dd * dd; }
        if (counted) xn -= x2;
        if (t.cam_dim[c] > 0) dn -= d2;
        if (g >= 0 && c == t.grp_cam[t.grp_off[g]]) {      // the group, once (Ceres counts a block some residual uses)
            bool any = false;
            for (int e = t.grp_off[g]; e < t.grp_off[g + 1]; ++e) { const int c2 = t.grp_cam[e]; any = any || t.cam_obs_off[c2 + 1] > t.cam_obs_off[c2]; }
            if (any) xn += x2;
            dn += d2;
        }
    }
    dn = wave_tree(dn); xn = wave_tree(xn);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = dn; sh[1][threadIdx.x >> 6] = xn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = scal[3] + (((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3]), b = scal[4] + (((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3]);
        scal[3] = a < 0.0 ? 0.0 : a;      // (rounding of the subtraction only; a NaN stays one)
        scal[4] = b < 0.0 ? 0.0 : b;
    }
}

}  // namespace

// ---- launchers (rcn_int_ba_solve, ba.hip; all on `st`)
hipError_t rcn_tied_scale(const Dev &t, const double *Uraw, double *sc, int jacobi, hipStream_t st)
{
    if (t.n_groups > 0) k_tied_scale<<<(4 * t.n_groups + 63) / 64, 64, 0, st>>>(t, Uraw, sc, jacobi);
    return hipGetLastError();
}
hipError_t rcn_tied_diag(const Dev &t, const double *Uraw, const double *sc, double *dgc, double lo, double hi, hipStream_t st)
{
    if (t.n_groups > 0) k_tied_diag<<<(4 * t.n_groups + 63) / 64, 64, 0, st>>>(t, Uraw, sc, dgc, lo, hi);
    return hipGetLastError();
}
hipError_t rcn_tied_fold(const Dev &t, const double *S, const double *rhs, double inv_radius, hipStream_t st)
{
    k_tied_fold_own<<<t.n, 256, 0, st>>>(t, S, rhs);
    if (t.n_groups > 0) {
        k_tied_fold_rows<<<dim3(t.n, t.n_groups), 64, 0, st>>>(t, S);
        k_tied_fold_groups<<<dim3(t.n_groups, t.n_groups + 2), 64, 0, st>>>(t, rhs, inv_radius);
    }
    return hipGetLastError();
}
hipError_t rcn_tied_expand(const Dev &t, const double *x, double *out, hipStream_t st)
{
    k_tied_expand<<<(t.n + 255) / 256, 256, 0, st>>>(t, x, out);
    return hipGetLastError();
}
hipError_t rcn_tied_gradmax(const Dev &t, const double *gcraw, const double *gpraw, int np, const double *intr, double *out, hipStream_t st)
{
    const int work = std::max(std::max(t.nc, 4 * t.n_groups), 3 * np);
    k_tied_gradmax<<<std::max(1, std::min(1024, (work + 255) / 256)), 256, 0, st>>>(t, gcraw, gpraw, 3 * np, intr, out);
    return hipGetLastError();
}
hipError_t rcn_tied_norms(const Dev &t, const double *intr, const double *intr2, double *scal, hipStream_t st)
{
    k_tied_norms<<<1, 256, 0, st>>>(t, intr, intr2, scal);
    return hipGetLastError();
}
