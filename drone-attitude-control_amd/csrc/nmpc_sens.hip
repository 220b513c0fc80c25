// nmpc_sens.hip — solution sensitivities of the batched LQ-OCP solve (nmpc_sens_forward / nmpc_sens_adjoint).
//
// At an accepted active set S the solution is z = z_0 + W[:, S] nu, W_SS nu = b_S - z_0,S (nmpc_api.cpp
// lqr_wmat), z_0 = T_x x0 + V_y yref + v_c the unconstrained solution. On the region where S holds
//
//   dz/dx0 = T_x - W[:, S] W_SS^-1 T_x[S, :]                                   (forward, ne x nx)
//   J' g   : g~ = g - E_S' W_SS^-1 (W[S, :] g);  grad_x0 = T_x' g~;  grad_yref = V_y' g~     (adjoint)
//
// W is the projected inverse Hessian itself (lqr_wmat: column e' is minus the minimiser for a unit gradient at
// e', i.e. +H^-1 e' on the feasible subspace): positive semidefinite, so the kernels factor W_SS = L L'.
//
// Mapping: one wavefront per instance, instances by a static stride over the grid's wavefronts (no counter,
// no atomics, no wait of any kind: wavefronts never exchange data, every loop is bounded by ne, the set size
// or the batch). Per instance:
//   1. the active set, read from the stored solution with the lean loop's on-bound rule (nmpc_cl_fast.hip
//      ClfTol<double>::onb: z within 1e-7 (1 + |b|) of a bound), compacted in element order by ballot and
//      prefix count into LDS; x_0 is pinned and never a member. An empty set leaves here: the forward call
//      copies the stage's T_x rows, the adjoint is T_x' g and V_y' g.
//   2. W_SS gathered into LDS (lower triangle, packed by rows), right-looking Cholesky with a lane per
//      row. A pivot below 1e-9 of its original diagonal marks a bound that depends linearly on earlier ones:
//      its row and column are zeroed, its solution entry is zero, the instance's status is
//      NMPC_SENS_DEGENERATE (a one-sided derivative).
//   3. both triangular solves with every right-hand side at once: lane s keeps row s of the right-hand sides
//      in registers (forward: the nx columns of T_x[S, :]; adjoint: the one column W[S, :] g), the pivot row
//      is broadcast by v_readlane.
//   4. forward: out[r][c] = T_x[e_r][c] - sum_s W[e_r, S_s] Y[s][c] for the nz rows of the stage;
//      adjoint: g~ in LDS, then one lane per output column of [T_x | V_y]' g~, four instances per sweep
//      of the table.
// Every sum has a fixed order and there are no floating-point atomics: two calls return the same bits.
// More than 64 on-bound elements: status NMPC_SENS_SET_TOO_LARGE and NaN outputs; a failed solve
// (status != 0): NMPC_SENS_NO_SOLUTION and NaN outputs.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "nmpc_internal.h"

namespace nmpc {
namespace sens {

constexpr int SMAX = 64;                       // largest active set (one lane per set row)
constexpr int TRI = SMAX * (SMAX + 1) / 2;     // packed lower triangle
constexpr int WPB = 2;                         // wavefronts per workgroup
constexpr int AIB = 4;                         // adjoint: instances per wavefront pass
constexpr double ONB = 1e-7;                   // on-bound threshold (ClfTol<double>::onb)
constexpr double PIV = 1e-9;                   // dependent-bound pivot threshold, relative to the original diagonal

#define SENS_SYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)

// lane k's value in every lane (k the same in every lane: v_readlane)
__device__ __forceinline__ double bcast(double v, int k)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}
// the wavefront's sum in every lane, fixed order
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int tri(int i, int j) { return ((i * (i + 1)) >> 1) + j; }   // j <= i

template <int NRHS>
struct WaveLds {
    double L[TRI];               // Cholesky factor of W_SS, packed lower triangle
    double Y[SMAX][NRHS];        // the set solve's solution
    int S[SMAX];                 // the active elements, in element order
};

// the solution's element e = k nz + r of instance b
template <int NX, int NU>
__device__ __forceinline__ double z_at(const SensParams &p, int b, int e)
{
    constexpr int NZ = NX + NU;
    const int k = e / NZ, r = e - k * NZ;
    return r < NX ? p.x[((size_t)b * (p.N + 1) + k) * NX + r] : p.u[((size_t)b * p.N + k) * NU + (r - NX)];
}

// the active set of instance b into lds.S (element order); returns its size (> SMAX: only the first SMAX stored)
template <int NX, int NU, int NRHS>
__device__ int active_set(const SensParams &p, int b, int lane, WaveLds<NRHS> &lds)
{
    constexpr int NZ = NX + NU;
    int cnt = 0;
    for (int e0 = 0; e0 < p.ne; e0 += 64) {
        const int e = e0 + lane, k = e / NZ, r = e - k * NZ;
        bool on = false;
        if (e < p.ne && !(k == 0 && r < NX) && !(k == p.N && r >= NX)) {
            const int ty = k == 0 ? 0 : (k == p.N ? 2 : 1);
            const double l = p.lbnd[ty * NZ + r], u = p.ubnd[ty * NZ + r], z = z_at<NX, NU>(p, b, e);
            on = (fabs(l) < 1e20 && z <= l + ONB * (1.0 + fabs(l))) || (fabs(u) < 1e20 && z >= u - ONB * (1.0 + fabs(u)));
        }
        const unsigned long long m = __ballot(on);
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (on && pos < SMAX) lds.S[pos] = e;
        cnt += __popcll(m);
    }
    SENS_SYNC();
    return cnt;
}

// W_SS -> L L' in lds.L (lane = row); returns the mask of the dropped (dependent) set rows
template <int NRHS>
__device__ unsigned long long factor(const SensParams &p, int n, int lane, WaveLds<NRHS> &lds)
{
    const int ei = lane < n ? lds.S[lane] : 0;
    double d0 = 1.0;
    if (lane < n) {
        for (int j = 0; j <= lane; j++) {
            const double a = p.W[(size_t)lds.S[j] * p.ne + ei];
            lds.L[tri(lane, j)] = a;
            if (j == lane) d0 = a;
        }
    }
    SENS_SYNC();
    unsigned long long dropped = 0;
    for (int k = 0; k < n; k++) {
        const double d = lds.L[tri(k, k)], dk0 = bcast(d0, k);
        SENS_SYNC();   // (every lane has read the pivot before lane k rewrites it)
        if (!(d > PIV * dk0) || !(dk0 > 0.0)) {
            // bound k depends on the earlier ones: out of the set (row and column zero, unit pivot)
            dropped |= 1ull << k;
            if (lane == k) {
                for (int j = 0; j < k; j++) lds.L[tri(k, j)] = 0.0;
                lds.L[tri(k, k)] = 1.0;
            }
            if (lane > k && lane < n) lds.L[tri(lane, k)] = 0.0;
            SENS_SYNC();
            continue;
        }
        const double s = sqrt(d);
        double lik = 0.0;
        if (lane == k) lds.L[tri(k, k)] = s;
        if (lane > k && lane < n) {
            lik = lds.L[tri(lane, k)] / s;
            lds.L[tri(lane, k)] = lik;
        }
        SENS_SYNC();
        // trailing update of row `lane`: L[i][j] -= L[i][k] L[j][k], k < j <= i
        if (lane > k && lane < n)
            for (int j = k + 1; j <= lane; j++) lds.L[tri(lane, j)] -= lik * lds.L[tri(j, k)];
        SENS_SYNC();
    }
    return dropped;
}

// (L L') y = r for NRHS columns, row `lane` of r in registers; a dropped row (unit pivot, zero row) gives y = 0
template <int NRHS>
__device__ void solve(int n, int lane, WaveLds<NRHS> &lds, double (&r)[NRHS])
{
    for (int k = 0; k < n; k++) {   // L y = r
        const double lkk = lds.L[tri(k, k)];
        const double lik = (lane > k && lane < n) ? lds.L[tri(lane, k)] : 0.0;
#pragma unroll
        for (int c = 0; c < NRHS; c++) {
            const double yk = bcast(r[c], k) / lkk;
            if (lane == k) r[c] = yk;
            r[c] -= lik * yk;
        }
    }
    for (int k = n - 1; k >= 0; k--) {   // L' x = y
        const double lkk = lds.L[tri(k, k)];
        const double lki = lane < k ? lds.L[tri(k, lane)] : 0.0;
#pragma unroll
        for (int c = 0; c < NRHS; c++) {
            const double xk = bcast(r[c], k) / lkk;
            if (lane == k) r[c] = xk;
            r[c] -= lki * xk;
        }
    }
}

template <int NX, int NU>
__global__ __launch_bounds__(64 * WPB) void sens_forward_kernel(SensParams p)
{
    constexpr int NZ = NX + NU;
    __shared__ WaveLds<NX> wl[WPB];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    WaveLds<NX> &lds = wl[wv];
    const int nwaves = gridDim.x * WPB;
    const int rows = p.stage < p.N ? NZ : NX, e_base = p.stage * NZ;
    const double nan = __builtin_nan("");
    for (int b = blockIdx.x * WPB + wv; b < p.B; b += nwaves) {
        double *ox = p.sens_x + (size_t)b * NX * NX, *ou = p.sens_u + (size_t)b * NU * NX;
        auto store = [&](int idx, double v) {   // idx = r * NX + c over the stage's rows
            if (idx < NX * NX) ox[idx] = v;
            else ou[idx - NX * NX] = v;
        };
        int st = NMPC_SENS_OK_, n = 0;
        if (p.status[b] != 0) st = NMPC_SENS_NO_SOLUTION_;
        else {
            n = active_set<NX, NU, NX>(p, b, lane, lds);
            if (n > SMAX) st = NMPC_SENS_SET_TOO_LARGE_;
        }
        if (st != NMPC_SENS_OK_) {
            for (int idx = lane; idx < NZ * NX; idx += 64) store(idx, nan);   // (stage N: sens_u NaN as well)
            if (lane == 0) p.sens_status[b] = st;
            SENS_SYNC();
            continue;
        }
        if (n == 0) {   // the common case: the stage's rows of T_x
            for (int idx = lane; idx < rows * NX; idx += 64) store(idx, p.tx[(size_t)e_base * NX + idx]);
            if (lane == 0) p.sens_status[b] = NMPC_SENS_OK_;
            SENS_SYNC();
            continue;
        }
        const unsigned long long dropped = factor<NX>(p, n, lane, lds);
        double r[NX];
        {
            // row `lane` of T_x[S, :]; a dropped row takes a zero right-hand side (its solution entry is zero)
            const bool live = lane < n && !((dropped >> lane) & 1ull);
            const int e = lane < n ? lds.S[lane] : 0;
#pragma unroll
            for (int c = 0; c < NX; c++) r[c] = live ? p.tx[(size_t)e * NX + c] : 0.0;
        }
        solve<NX>(n, lane, lds, r);
        if (lane < n) {
#pragma unroll
            for (int c = 0; c < NX; c++) lds.Y[lane][c] = r[c];
        }
        SENS_SYNC();
        for (int idx = lane; idx < rows * NX; idx += 64) {
            const int rr = idx / NX, c = idx - rr * NX, e = e_base + rr;
            double v = p.tx[(size_t)e * NX + c];
            for (int s = 0; s < n; s++) v -= p.W[(size_t)lds.S[s] * p.ne + e] * lds.Y[s][c];
            store(idx, v);
        }
        if (lane == 0) p.sens_status[b] = dropped ? NMPC_SENS_DEGENERATE_ : NMPC_SENS_OK_;
        SENS_SYNC();   // (the next instance rewrites S / L / Y)
    }
}

// AIB instances per wavefront pass: each instance's g~ is built in turn (its own set solve), then one sweep over
// [T_x | V_y] serves all of them — the table (1 MB for quad13 N = 20) is read from L2 once per AIB instances, and
// that read is what the adjoint's time is made of
template <int NX, int NU>
__global__ __launch_bounds__(64 * WPB) void sens_adjoint_kernel(SensParams p)
{
    constexpr int NZ = NX + NU;
    __shared__ WaveLds<1> wl[WPB];
    __shared__ double gall[WPB][AIB][SENS_GMAX];   // g~ over the elements, per instance of the pass
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    WaveLds<1> &lds = wl[wv];
    const int nwaves = gridDim.x * WPB;
    const int K = NX + p.ystride;
    const double nan = __builtin_nan("");
    for (int b0 = (blockIdx.x * WPB + wv) * AIB; b0 < p.B; b0 += nwaves * AIB) {
        int stv[AIB];   // per instance: its status, or -1 past the batch's end (all the same in every lane)
#pragma unroll
        for (int i = 0; i < AIB; i++) {
            const int b = b0 + i;
            double *g = gall[wv][i];
            int st = NMPC_SENS_OK_, n = 0;
            if (b >= p.B) st = -1;
            else if (p.status[b] != 0) st = NMPC_SENS_NO_SOLUTION_;
            else {
                n = active_set<NX, NU, 1>(p, b, lane, lds);
                if (n > SMAX) st = NMPC_SENS_SET_TOO_LARGE_;
            }
            stv[i] = st;
            if (st != NMPC_SENS_OK_) {   // nothing to pull back: a zero cotangent keeps the sweep below finite
                for (int e = lane; e < p.ne; e += 64) g[e] = 0.0;
                SENS_SYNC();
                continue;
            }
            // the cotangent over the elements (stage N has no inputs)
            for (int e = lane; e < p.ne; e += 64) {
                const int k = e / NZ, r = e - k * NZ;
                double v = 0.0;
                if (r < NX) v = p.seed_x[((size_t)b * (p.N + 1) + k) * NX + r];
                else if (k < p.N) v = p.seed_u[((size_t)b * p.N + k) * NU + (r - NX)];
                g[e] = v;
            }
            SENS_SYNC();
            if (n > 0) {
                const unsigned long long dropped = factor<1>(p, n, lane, lds);
                double r[1] = {0.0};
                for (int s = 0; s < n; s++) {   // W[S, :] g: column S_s of W (symmetric) against g
                    const double *wc = p.W + (size_t)lds.S[s] * p.ne;
                    double a = 0.0;
                    for (int e = lane; e < p.ne; e += 64) a += wc[e] * g[e];
                    a = wave_sum(a);
                    if (lane == s) r[0] = a;
                }
                if ((dropped >> lane) & 1ull) r[0] = 0.0;   // a dropped row: zero right-hand side
                solve<1>(n, lane, lds, r);
                if (lane < n) g[lds.S[lane]] -= r[0];   // g~ = g - E_S' W_SS^-1 (W[S, :] g)
                if (dropped) stv[i] = NMPC_SENS_DEGENERATE_;
                SENS_SYNC();   // (the next instance rewrites S / L)
            }
        }
        // [T_x | V_y]' g~ for the pass's instances: one lane per output column, each table word used AIB times
        for (int q = lane; q < K; q += 64) {
            double a[AIB];
#pragma unroll
            for (int i = 0; i < AIB; i++) a[i] = 0.0;
            const double *col = q < NX ? p.tx + q : p.vy + (q - NX);
            const size_t ld = q < NX ? (size_t)NX : (size_t)p.ystride;
            for (int e = 0; e < p.ne; e++) {
                const double v = col[(size_t)e * ld];
#pragma unroll
                for (int i = 0; i < AIB; i++) a[i] += v * gall[wv][i][e];
            }
#pragma unroll
            for (int i = 0; i < AIB; i++) {
                if (stv[i] < 0) continue;
                const size_t b = (size_t)(b0 + i);
                const double v = stv[i] >= NMPC_SENS_NO_SOLUTION_ ? nan : a[i];
                if (q < NX) p.grad_x0[b * NX + q] = v;
                else p.grad_yref[b * p.ystride + (q - NX)] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < AIB; i++)
            if (lane == 0 && stv[i] >= 0) p.sens_status[b0 + i] = stv[i];
        SENS_SYNC();   // (the next pass rewrites the cotangents)
    }
}

template <class F>
static bool dispatch(int nx, int nu, F &&f)
{
    if (nx == 4 && nu == 2) f(sens_forward_kernel<4, 2>, sens_adjoint_kernel<4, 2>);
    else if (nx == 6 && nu == 2) f(sens_forward_kernel<6, 2>, sens_adjoint_kernel<6, 2>);
    else if (nx == 13 && nu == 4) f(sens_forward_kernel<13, 4>, sens_adjoint_kernel<13, 4>);
    else return false;
    return true;
}

}  // namespace sens

bool sens_shape(int nx, int nu)
{
    return sens::dispatch(nx, nu, [](auto, auto) {});
}

int sens_resident(int nx, int nu, int adjoint, int device)
{
    int res = 0;
    sens::dispatch(nx, nu, [&](auto kf, auto ka) {
        int per_cu = 0, cus = 0;
        const hipError_t e = adjoint ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ka, 64 * sens::WPB, 0)
                                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kf, 64 * sens::WPB, 0);
        if (e != hipSuccess || per_cu < 1) return;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) return;
        res = per_cu * cus;
    });
    return res;
}

hipError_t sens_launch(int nx, int nu, int adjoint, const SensParams &p, int resident, hipStream_t s)
{
    if (p.B < 1 || p.ne > SENS_GMAX || p.stage < 0 || p.stage > p.N) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    sens::dispatch(nx, nu, [&](auto kf, auto ka) {
        const int per = sens::WPB * (adjoint ? sens::AIB : 1);   // instances per workgroup pass
        const int blocks = std::max(1, std::min((p.B + per - 1) / per, std::max(1, resident)));
        if (adjoint) NMPC_LAUNCH(ka, dim3(blocks), dim3(64 * sens::WPB), 0, s, p);
        else NMPC_LAUNCH(kf, dim3(blocks), dim3(64 * sens::WPB), 0, s, p);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace nmpc
