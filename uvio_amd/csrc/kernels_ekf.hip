// StateHelper::EKFUpdate (StateHelper.cpp:116-197) for a direct (uncompressed) batch of r rows, as three
// launches whose products all run on the FP64 matrix cores (v_mfma_f64_16x16x4f64):
//
//   k_ekf_MS   grid:  M = P[:, I] H^T (N x r; one 16-row block per workgroup, the P rows gathered once
//                     into LDS) and S_up = H P_II H^T + s2 I = H T^T (one upper 16x16 tile pair per wave), with
//                     T = H P_II read from the batch's chi2 gate in the same launch, or gathered from the rows
//                     I of this update's own M in a second launch
//   k_ekf_fact one workgroup: LDL^T of [S ; r^T] in LDS with the unit-lower inverse alongside (dense_lds.h
//                     ldl_wave) -> L^-1, y = L^-1 r, and StateHelper::initialize's chi2 gate on y; its DENSE_R
//                     instances add a caller's dense R to S and gate on the pivots too (launch_ekf_update_R)
//   k_ekf_WP   grid over the upper 16x16 tile pairs (bi <= bj) of P: W_b = M_b L^-T for both row blocks
//                     (a GEMM with the explicit inverse, recomputed per tile pair instead of a separate
//                     launch), P_ij -= W_bi W_bj^T (written to both triangles), dx = W y on diagonal tiles
//
// The reference computes K = P H^T S^-1 through an LLT solve and P -= K M^T; here P -= (M L^-T)(M L^-T)^T
// and dx = (M L^-T)(L^-1 r): the same update (S = L L^T), every product on MFMA tiles.  The earlier chain
// (k_ekf_M, k_ekf_S, k_ekf_small, k_trinv16, k_trsm_lt, k_ekf_P: six launches, VALU tiles for the four
// products) cost 96 us per update at cfg2 in rocprof (profiles/r01g_cfg2_per_frame.txt).
//
// Also here: the delayed-initialization candidate (k_di_M, k_di_S, k_chain_apply) and the device chains of small
// measurements, UWB ranges, position fixes and pose fixes: a row kernel (k_uwb_row / k_fix_rows / k_pose_rows), then
// k_chain_M and k_chain_update<RangeGate | FixGate<R>> for all three.
//
// MFMA operand layout (f64 16x16x4): A (16x4) lane l holds A[l & 15][l >> 4]; B (4x16) lane l holds
// B[l >> 4][l & 15]; C/D register q of lane l is D[(l >> 4) + 4 q][l & 15].
#include <algorithm>
#include <stdexcept>

#include "dense_lds.h"
#include "kernels.h"

namespace uvhp {

// ---------------------------------------------------------------------------------------------------
// K1, two parts: M (blocks 0 .. nbM-1) and the upper tile pairs of S_up (blocks nbM ..; 8 pairs each).  Tall is
// non-null whenever a block index reaches nbM or beyond: a launch without it has exactly nbM blocks.
// km (optional, with Tall: a SLAM chunk): the k-step mask of every 16-row tile of H (kernels.h DBatchParams::kmask).
// Column tile t of M and the S tile pairs (a, b) have H's row tile t / a as an operand, so their chains visit only
// its set steps (dense_lds.h tile_chain_masked: the same values).
constexpr int kMSThreads = 512;  // 8 waves: one M column tile / one S tile pair per wave at cfg2's r ~ 100
__global__ void __launch_bounds__(kMSThreads) k_ekf_MS(const double *__restrict__ P, int ldp, int N,
                                                const double *__restrict__ H, int ldh, int r, int n,
                                                const int *__restrict__ hidx, double s2, double *__restrict__ M,
                                                double *__restrict__ Sup, int nbM, int *zero,
                                                const double *__restrict__ Tall, int ldt,
                                                const unsigned long long *__restrict__ km) {
  extern __shared__ double sh[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  if (zero && blockIdx.x == 0 && threadIdx.x == 0) *zero = 0;  // the update's negative-diagonal count
  if ((int)blockIdx.x < nbM) {
    // M rows i0 .. i0+15: Ps[i][k] = P[i0 + i][hidx[k]] staged once, each wave takes column tiles of M
    const int i0 = blockIdx.x * 16, lds = n | 1;
    double *Ps = sh;
    staged_copy(
        16 * n,
        [&](int e) {
          const int i = e / n, k = e - i * n;
          return (i0 + i < N) ? P[(size_t)(i0 + i) * ldp + hidx[k]] : 0.0;
        },
        [&](int e, double v) {
          const int i = e / n, k = e - i * n;
          Ps[i * lds + k] = v;
        });
    __syncthreads();
    const int nct = (r + 15) / 16;
    for (int t = wid; t < nct; t += kMSThreads / 64) {
      const int j0 = 16 * t, jr = j0 + r16;
      const double *Hr = H + (size_t)min(jr, r - 1) * ldh;
      const bool jv = jr < r;
      dbl4 acc = {0.0, 0.0, 0.0, 0.0};
      auto la = [&](int k) { return Ps[r16 * lds + k]; };
      auto lb = [&](int k) { return jv ? Hr[k] : 0.0; };
      if (km)
        acc = tile_chain_masked<16>(kmask_uniform(km[2 * t]), kmask_uniform(km[2 * t + 1]), n, kq, la, lb, acc);
      else
        acc = tile_chain<16>(0, n, kq, la, lb, acc);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int row = i0 + kq + 4 * q, col = j0 + r16;
        if (row < N && col < r) M[(size_t)row * r + col] = acc[q];
      }
    }
    return;
  }
  // T = H P_II is already in HBM from the batch's chi2 gate (k_gemm_HPg, rejected features' rows zeroed
  // there with their H rows), so S_up[a][b] = H_a T_b^T directly: one upper tile pair (a <= b) per wave,
  // one chain of loads instead of forming T_b first (same products, same ascending k order).
  // ldt < 0: Tall is this update's M = P[:, I] H^T (N x r, launched after the M blocks), whose rows hidx are
  // T^T: T[b][k] = M[hidx[k]][b].
  const bool gath = ldt < 0;
  int *hs = (int *)sh;
  if (gath) {
    for (int k = threadIdx.x; k < n; k += blockDim.x) hs[k] = hidx[k];
    __syncthreads();
  }
  const int nt = (r + 15) / 16;
  const int pair = (blockIdx.x - nbM) * (kMSThreads / 64) + wid;
  if (pair >= nt * (nt + 1) / 2) return;
  int at, bt;
  upper_pair(pair, nt, at, bt);
  const int ar = 16 * at + r16, br = 16 * bt + r16;
  const double *Ha = H + (size_t)min(ar, r - 1) * ldh;
  const double *Tb = gath ? Tall + min(br, r - 1) : Tall + (size_t)min(br, r - 1) * ldt;
  const bool av = ar < r, bv = br < r;
  dbl4 acc = {0.0, 0.0, 0.0, 0.0};
  auto la = [&](int k) { return av ? Ha[k] : 0.0; };
  auto lb = [&](int k) { return bv ? (gath ? Tb[(size_t)hs[k] * r] : Tb[k]) : 0.0; };
  if (km)
    acc = tile_chain_masked<16>(kmask_uniform(km[2 * at]), kmask_uniform(km[2 * at + 1]), n, kq, la, lb, acc);
  else
    acc = tile_chain<16>(0, n, kq, la, lb, acc);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int row = 16 * at + kq + 4 * q, col = 16 * bt + r16;
    if (row < r && col < r) Sup[(size_t)row * r + col] = acc[q] + (row == col ? s2 : 0.0);
  }
}

// initialize_invertible's M has at most this many columns (k_di_M's GEMV accumulators)
constexpr int kSmallMRows = 4;
// the M blocks' 16 x (n | 1) doubles; the gathered S blocks' n ints fit inside them
static size_t ekf_ms_lds_bytes(int n) { return (size_t)16 * (n | 1) * sizeof(double); }

// ---------------------------------------------------------------------------------------------------
// K2: one workgroup.  [S ; r^T] (S from the upper triangle of S_up = selfadjointView<Upper>,
// StateHelper.cpp:160) -> LDL^T with the unit-lower inverse alongside (dense_lds.h ldl_wave), then
// L^-1 = D^-1/2 L_u^-1 (lower, zeros above, ld r) into Linv_out and y = L^-1 r = D^1/2 (D^-1 L_u^-1 r).
// chi2_gate: StateHelper::initialize's test (StateHelper.cpp:458-470) on this factor: chi2 = |y|^2 in a
// fixed order against thr -> *chi2_gate (the P-update gate) and [chi2, accepted] into gate_out[0..1].
// LDS: the factor in LDS (a compile-time choice, so every access of the factorization is a DS instruction;
// a runtime choice makes them all FLAT)
// W: the panel waves of ldl_wave_inv (panel rows 16 + 48 W); one workgroup of kFactThreads.
// DENSE_R: a caller's dense noise matrix (launch_ekf_update_R): S = S_up + R, where S_up = H P_II H^T comes from
// k_ekf_MS with s2 = 0 and only R's upper triangle (r x r, ld ldr, device) is read, as the reference's
// S.triangularView<Upper>() += R (StateHelper.cpp:156).  With R = s2 I the staged values are k_ekf_MS's own
// (acc + 0.0) + s2, so the factor, L^-1 and y are the plain instance's bit for bit.
// The two gates differ, and are kept apart on purpose:
//   plain  optional (chi2_gate may be null); accepted = incoming *chi2_gate (the feature's linearization
//          succeeded) && !(chi2 > thr), so a NaN chi2 passes
//   dense  mandatory, the incoming value is not read; a caller's R can make S indefinite, so every pivot Dd[k] has
//          to be finite and > 0 and chi2 finite: accepted = pivots_ok && isfinite(chi2) && !(chi2 > thr), chi2
//          written as NaN when a pivot is bad
// Both: accepted -> *chi2_gate (k_ekf_WP's gate), [chi2, accepted] -> gate_out[0..1].
template <int W, bool LDS, bool DENSE_R>
__global__ void __launch_bounds__(kFactThreads) k_ekf_fact(const double *__restrict__ Sup, int r,
                                                  const double *__restrict__ R, int ldr,
                                                  const double *__restrict__ res, int res_stride,
                                                  double *__restrict__ Linv_out, double *__restrict__ y_out, double *Sg,
                                                  int *chi2_gate, double chi2_thr, double *__restrict__ gate_out) {
  extern __shared__ double lds[];
  double *A = LDS ? lds : Sg;
  const int ld = r | 1;  // odd row stride: conflict-free 64-bit LDS reads down a column
  double *Dd = A + (size_t)(r + 1) * ld, *sd = Dd + r;
  staged_copy(
      r * r + r,
      [&](int e) {
        if (e >= r * r) return res[(size_t)(e - r * r) * res_stride];
        const int a = e / r, b = e - a * r;
        if constexpr (DENSE_R)
          return (b <= a) ? Sup[(size_t)b * r + a] + R[(size_t)b * ldr + a] : 0.0;
        else
          return (b <= a) ? Sup[(size_t)b * r + a] : 0.0;
      },
      [&](int e, double v) {
        if (e >= r * r) {
          A[(size_t)r * ld + e - r * r] = v;
        } else {
          const int a = e / r, b = e - a * r;
          if (b <= a) A[(size_t)a * ld + b] = v;
        }
      });
  __syncthreads();
  ldl_wave_inv<1, SqLayout, W>(A, SqLayout{ld}, r, r + 1, Dd, true);
  for (int k = threadIdx.x; k < r; k += blockDim.x) {
    const double q = sqrt(Dd[k]);
    sd[k] = q;
    y_out[k] = A[(size_t)r * ld + k] * q;
  }
  __syncthreads();
  if ((DENSE_R || chi2_gate) && threadIdx.x < 64) {
    // chi2 = |y|^2: strided by 64, then the wavefront's halves added down to lane 0
    double s = 0.0;
    int ok = 1;  // dense: every pivot finite and positive
    for (int k = threadIdx.x; k < r; k += 64) {
      const double v = A[(size_t)r * ld + k] * sd[k];
      if constexpr (DENSE_R) {
        const double d = Dd[k];
        ok &= (isfinite(d) && d > 0.0) ? 1 : 0;
      }
      s += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_down(s, o, 64);
      if constexpr (DENSE_R) ok &= __shfl_down(ok, o, 64);
    }
    if (threadIdx.x == 0) {
      int acc;
      if constexpr (DENSE_R)
        acc = ok && isfinite(s) && !(s > chi2_thr);
      else
        acc = (*chi2_gate != 0) && !(s > chi2_thr);
      *chi2_gate = acc;
      gate_out[0] = (!DENSE_R || ok) ? s : __builtin_nan("");
      gate_out[1] = acc;
    }
  }
  for (int e = threadIdx.x; e < r * r; e += blockDim.x) {
    const int a = e / r, b = e - a * r;
    double v = 0.0;
    if (b < a)
      v = A[(size_t)b * ld + a] / sd[a];
    else if (b == a)
      v = 1.0 / sd[a];
    Linv_out[e] = v;
  }
}
size_t ekf_small_lds_bytes(int r) { return (dense_lds_bytes(r + 1, r) + (size_t)2 * r * sizeof(double)); }

// ---------------------------------------------------------------------------------------------------
// K3: tile pair (bi, bj), bi <= bj, of the nb x nb tile grid of P (blocks enumerated row by row)
__global__ void __launch_bounds__(256) k_ekf_WP(double *__restrict__ P, int ldp, int N, const double *__restrict__ M,
                                                int r, const double *__restrict__ Linv, const double *__restrict__ y,
                                                double *__restrict__ dx, int *neg, const int *gate, int nb) {
  if (gate && *gate == 0) return;  // no accepted rows: the reference makes no update
  extern __shared__ double sh[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  int bi, bj;
  upper_pair(blockIdx.x, nb, bi, bj);
  const int ldw = r | 1;
  double *Wi = sh, *Wj = sh + 16 * ldw, *red = sh + 32 * ldw;
  // this thread's P element, fetched before the products so its latency is hidden
  const int ei = threadIdx.x >> 4, ej = threadIdx.x & 15;
  const int gi = 16 * bi + ei, gj = 16 * bj + ej;
  const bool pw = gi < N && gj < N && (bi < bj || ej >= ei);
  const double pv = pw ? P[(size_t)gi * ldp + gj] : 0.0;
  // W_b[i][c] = sum_{k <= c} M[16 b + i][k] Linv[c][k]
  const int nct = (r + 15) / 16, ntask = (bi == bj ? 1 : 2) * nct;
  for (int t = wid; t < ntask; t += 4) {
    const int which = t / nct, ct = t - which * nct;
    double *Wd = which ? Wj : Wi;
    const int row = 16 * (which ? bj : bi) + r16, c = 16 * ct + r16;
    const double *Mr = M + (size_t)min(row, N - 1) * r;
    const double *Lr = Linv + (size_t)min(c, r - 1) * r;
    const bool rv = row < N, cv = c < r;
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = tile_chain(
        0, min(16 * ct + 16, r), kq, [&](int k) { return rv ? Mr[k] : 0.0; }, [&](int k) { return cv ? Lr[k] : 0.0; },
        acc);
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (cv) Wd[(kq + 4 * q) * ldw + c] = acc[q];
  }
  __syncthreads();
  const double *Wb = (bi == bj) ? Wi : Wj;
  dbl4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 4 * wid; k0 < r; k0 += 16) {  // wave w: k-slabs w, w + 4, ...
    const int k = k0 + kq;
    const double a = (k < r) ? Wi[r16 * ldw + k] : 0.0;
    const double bb = (k < r) ? Wb[r16 * ldw + k] : 0.0;
    acc = mfma4(a, bb, acc);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) red[wid * 256 + (kq + 4 * q) * 16 + r16] = acc[q];
  __syncthreads();
  if (pw) {
    const int e = threadIdx.x;
    const double s = (red[e] + red[256 + e]) + (red[512 + e] + red[768 + e]);
    const double v = pv - s;
    P[(size_t)gi * ldp + gj] = v;
    P[(size_t)gj * ldp + gi] = v;
    if (gi == gj && v < 0.0) atomicAdd(neg, 1);
  }
  if (bi == bj && wid == 1) {
    const int i = lane >> 2, part = lane & 3;
    double a = 0.0;
    for (int k = part; k < r; k += 4) a += Wi[i * ldw + k] * y[k];
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (part == 0 && 16 * bi + i < N) dx[16 * bi + i] = a;
  }
}

// Thread t of one workgroup moves clone t (t < ncl) or camera t - ncl by dx: Var::update (PoseJPL: quat_boxplus,
// p += dp; intrinsics +=) and the tables' rotation matrices (quat_2_Rot), the host's formulas
__device__ void chain_tables_apply(int t, const double *__restrict__ dx, DClone *__restrict__ clones,
                                   DPoseVal *__restrict__ cv, int ncl, DCam *__restrict__ cams,
                                   DPoseVal *__restrict__ camv, int ncam, int calib_ext, int calib_intr) {
  if (t < ncl) {  // PoseJPL::update of clone t, then the table's R_GtoI / p_IinG
    DPoseVal &v = cv[t];
    const double *d = dx + v.pid;
    quat_boxplus(v.q, d);
    for (int k = 0; k < 3; k++) v.p[k] += d[3 + k];
    quat_2_Rot(v.q, clones[t].R);
    for (int k = 0; k < 3; k++) clones[t].p[k] = v.p[k];
  } else if (t < ncl + ncam) {
    const int c = t - ncl;
    DCam &dc = cams[c];
    if (calib_ext && dc.pid_ext >= 0) {
      DPoseVal &v = camv[c];
      const double *d = dx + v.pid;
      quat_boxplus(v.q, d);
      for (int k = 0; k < 3; k++) v.p[k] += d[3 + k];
      quat_2_Rot(v.q, dc.R_ItoC);
      for (int k = 0; k < 3; k++) dc.p_IinC[k] = v.p[k];
    }
    if (calib_intr && dc.pid_intr >= 0)
      for (int k = 0; k < 8; k++) dc.cam.v[k] += dx[dc.pid_intr + k];
  }
}

// Delayed-initialization chain step (kernels.h launch_chain_apply).  Block 0 updates the tables (one thread
// per clone / camera) when the candidate was accepted; every block clears a rejected candidate's slot of D rows and
// columns (D: the landmark dimension, 3 or 1).
template <int D>
__global__ void __launch_bounds__(256) k_chain_apply(const DFeatOut *__restrict__ fout, const int *__restrict__ gate,
                                                     const int *__restrict__ neg, const double *__restrict__ dx,
                                                     DClone *__restrict__ clones, DPoseVal *__restrict__ cv, int ncl,
                                                     DCam *__restrict__ cams, DPoseVal *__restrict__ camv, int ncam,
                                                     int calib_ext, int calib_intr, double *__restrict__ xv, int Nx,
                                                     double *__restrict__ P, int ldp, int Ntot, int slot,
                                                     double *__restrict__ out) {
  const bool acc = (!fout || fout->status == 0) && (!gate || *gate != 0);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (!acc) {
    if (slot >= 0)
      for (int e = t; e < D * Ntot; e += gridDim.x * blockDim.x) {
        const int i = e / D, a = e - D * i;
        P[(size_t)(slot + a) * ldp + i] = 0.0;
        P[(size_t)i * ldp + slot + a] = 0.0;
      }
  } else if (dx && xv) {  // the additive mirror (landmarks): Var::update of a vector, val += dx
    for (int e = t; e < Nx; e += gridDim.x * blockDim.x) xv[e] += dx[e];
  }
  if (acc && blockIdx.x == 0 && dx) chain_tables_apply(t, dx, clones, cv, ncl, cams, camv, ncam, calib_ext, calib_intr);
  if (t == 0) {
    out[0] = acc ? 1.0 : 0.0;
    out[1] = neg ? (double)*neg : 0.0;
  }
}

void launch_chain_apply(hipStream_t s, const DFeatOut *fout, const int *gate, const int *neg, const double *dx,
                        DClone *clones, DPoseVal *cv, int ncl, DCam *cams, DPoseVal *camv, int ncam, int calib_ext,
                        int calib_intr, double *xv, int Nx, double *P, int ldp, int Ntot, int slot, double *out, int d) {
  if (ncl + ncam > 256) throw std::runtime_error("update chain: more clones + cameras than one workgroup");
  if (d != 3 && d != 1) throw std::runtime_error("update chain: landmark dimension " + std::to_string(d));
  const int nb = std::max(1, std::min(16, (std::max(3 * Ntot, Nx) + 255) / 256));
  hipLaunchKernelGGL(d == 3 ? k_chain_apply<3> : k_chain_apply<1>, dim3(nb), dim3(256), 0, s, fout, gate, neg, dx, clones,
                     cv, ncl, cams, camv, ncam, calib_ext, calib_intr, xv, Nx, P, ldp, Ntot, slot, out);
}

// ---------------------------------------------------------------------------------------------------
// Device chains of small measurements (kernels.h DChainRegion / DChainRow): per step a row kernel, k_chain_M,
// k_chain_update.
// The head of a row kernel.  A negative covariance diagonal in an earlier step halts the rest of the chain: the
// reference stops at that update (StateHelper.cpp:181, std::exit), so no later step may touch P (the host then
// reports E_NUMERIC).  Returns the previous step's dx when the state has to move by it (accepted and not halted),
// else null; prev is null for the chain's first step.
__device__ const double *chain_prev_dx(const DChainRegion *prev, bool &halt) {
  halt = false;
  if (!prev) return nullptr;
  halt = prev->neg > 0 || prev->halt != 0;
  return (prev->accepted != 0.0 && !halt) ? prev->dx : nullptr;
}
__device__ void chain_reset(DChainRegion *region, bool halt) {
  region->accepted = 0.0;
  region->neg = 0;
  region->halt = halt ? 1 : 0;
  region->chi2 = region->extra = 0.0;
}

// Chained UWB ranges (kernels.h DUwbState)
__global__ void k_uwb_row(DUwbState *st, int j, const DChainRegion *__restrict__ prev, DChainRow *__restrict__ row,
                          DChainRegion *__restrict__ region) {
  if (threadIdx.x != 0) return;
  DUwbState &u = *st;
  bool halt;
  if (const double *dx = chain_prev_dx(prev, halt)) {
    // Var::update of the previous range's dx (engine_state.cpp): IMU quaternion boxplus + position, p_IinU and
    // the anchors additive
    quat_boxplus(u.q, dx + u.id_imu);
    for (int k = 0; k < 3; k++) u.p[k] += dx[u.id_imu + 3 + k];
    if (u.id_cal >= 0)
      for (int k = 0; k < 3; k++) u.pU[k] += dx[u.id_cal + k];
    for (int a = 0; a < u.nr; a++)
      if (u.id_anc[a] >= 0)
        for (int k = 0; k < 5; k++) u.anc[a][k] += dx[u.id_anc[a] + k];
  }
  const bool cal = u.id_cal >= 0, anc = u.id_anc[j] >= 0;
  double h[kChainMaxCols + 1];
  const int n = uwb_row(u.q, u.p, u.pU, u.anc[j], cal, anc, u.range[j], h);
  DChainRow &o = *row;
  for (int k = 0; k < n; k++) {
    o.H[0][k] = h[k];
    // the columns [IMU (6), p_IinU (3) if calibrated, anchor (5) if free]
    o.hidx[k] = k < 6 ? u.id_imu + k : (cal && k < 9) ? u.id_cal + k - 6 : u.id_anc[j] + k - (cal ? 9 : 6);
  }
  o.res[0] = h[n];
  o.R[0] = u.s2;
  o.thr = u.thr;
  o.n = n;
  o.pad = 0;
  chain_reset(region, halt);
}

void launch_uwb_row(hipStream_t s, DUwbState *st, int j, const DChainRegion *prev, DChainRow *row,
                    DChainRegion *region) {
  hipLaunchKernelGGL(k_uwb_row, dim3(1), dim3(64), 0, s, st, j, prev, row, region);
}

// Chained position fixes (kernels.h DFixState)
__global__ void k_fix_rows(DFixState *st, int j, const DChainRegion *__restrict__ prev, DChainRow *__restrict__ row,
                           DChainRegion *__restrict__ region) {
  if (threadIdx.x != 0) return;
  DFixState &u = *st;
  bool halt;
  if (const double *dx = chain_prev_dx(prev, halt)) {
    // Var::update of the previous fix's dx: IMU quaternion boxplus + position, the aux lever arms additive
    quat_boxplus(u.q, dx + u.id_imu);
    for (int k = 0; k < 3; k++) u.p[k] += dx[u.id_imu + 3 + k];
    for (int a = 0; a < u.nf; a++)
      if (u.id_aux[a] >= 0)
        for (int k = 0; k < 3; k++) u.s[a][k] += dx[u.id_aux[a] + k];
  }
  const int r = u.r[j];
  const bool aux = u.id_aux[j] >= 0;
  const double *s = u.s[j], *C = u.C[j];
  double Rm[9], Sx[9], A[9], pred[3];
  quat_2_Rot(u.q, Rm);   // R_GtoI
  m3t_vec(Rm, s, pred);  // R_GtoI^T s
  for (int k = 0; k < 3; k++) pred[k] += u.p[k];
  skew(s, Sx);
  m3_mul_at(Rm, Sx, A);  // R_GtoI^T [s]x
  DChainRow &o = *row;
  for (int a = 0; a < 3; a++) {
    for (int k = 0; k < 9; k++) o.H[a][k] = 0.0;
    o.res[a] = 0.0;
    if (a >= r) continue;
    const double *c = C + 3 * a;
    for (int k = 0; k < 3; k++) {
      o.H[a][k] = -(c[0] * A[k] + c[1] * A[3 + k] + c[2] * A[6 + k]);
      o.H[a][3 + k] = c[k];
      if (aux) o.H[a][6 + k] = c[0] * Rm[3 * k] + c[1] * Rm[3 * k + 1] + c[2] * Rm[3 * k + 2];
    }
    o.res[a] = u.z[j][a] - dot3(c, pred);
  }
  for (int k = 0; k < 9; k++) {
    o.R[kChainMaxRows * (k / 3) + k % 3] = u.R[j][k];
    o.hidx[k] = k < 6 ? u.id_imu + k : (aux ? u.id_aux[j] + k - 6 : 0);
  }
  o.thr = u.thr[j];
  o.n = aux ? 9 : 6;
  o.pad = 0;
  chain_reset(region, halt);
}

void launch_fix_rows(hipStream_t s, DFixState *st, int j, const DChainRegion *prev, DChainRow *row,
                     DChainRegion *region) {
  hipLaunchKernelGGL(k_fix_rows, dim3(1), dim3(64), 0, s, st, j, prev, row, region);
}

// Chained pose fixes (kernels.h DPoseState)
__global__ void k_pose_rows(DPoseState *st, int j, const DChainRegion *__restrict__ prev, DChainRow *__restrict__ row,
                            DChainRegion *__restrict__ region) {
  if (threadIdx.x != 0) return;
  DPoseState &u = *st;
  bool halt;
  if (const double *dx = chain_prev_dx(prev, halt)) {
    // Var::update of the previous fix's dx: IMU quaternion boxplus + position, the aux lever arms additive, the aux
    // mounting rotations by boxplus.  Two fixes that name one variable carry equal copies, which move alike.
    quat_boxplus(u.q, dx + u.id_imu);
    for (int k = 0; k < 3; k++) u.p[k] += dx[u.id_imu + 3 + k];
    for (int a = 0; a < u.nf; a++) {
      if (u.id_arm[a] >= 0)
        for (int k = 0; k < 3; k++) u.s[a][k] += dx[u.id_arm[a] + k];
      if (u.id_rot[a] >= 0) quat_boxplus(u.qS[a], dx + u.id_rot[a]);
    }
  }
  const int r = u.r[j];
  const bool arm = u.id_arm[j] >= 0, rot = u.id_rot[j] >= 0;
  const int c_arm = 6, c_rot = arm ? 9 : 6, n = c_rot + (rot ? 3 : 0);
  const double *s = u.s[j];
  double Rm[9], RS[9], qp[4], qi[4], dq[4];
  quat_2_Rot(u.q, Rm);      // R_GtoI
  quat_2_Rot(u.qS[j], RS);  // R_ItoS
  quat_multiply(u.qS[j], u.q, qp);  // q_GtoS
  qi[0] = -qp[0], qi[1] = -qp[1], qi[2] = -qp[2], qi[3] = qp[3];
  quat_multiply(u.zq[j], qi, dq);  // w >= 0 (quat_multiply)
  DChainRow &o = *row;
  for (int a = 0; a < kChainMaxRows; a++) {
    for (int k = 0; k < kChainMaxCols; k++) o.H[a][k] = 0.0;
    o.res[a] = 0.0;
  }
  for (int a = 0; a < 3; a++) {
    for (int k = 0; k < 3; k++) o.H[a][k] = RS[3 * a + k];
    if (rot) o.H[a][c_rot + a] = 1.0;
    o.res[a] = 2.0 * dq[a];
  }
  if (r == 6) {
    double Sx[9], A[9], pred[3];
    m3t_vec(Rm, s, pred);  // R_GtoI^T s
    skew(s, Sx);
    m3_mul_at(Rm, Sx, A);  // R_GtoI^T [s]x
    for (int a = 0; a < 3; a++) {
      for (int k = 0; k < 3; k++) {
        o.H[3 + a][k] = -A[3 * a + k];
        if (arm) o.H[3 + a][c_arm + k] = Rm[3 * k + a];
      }
      o.H[3 + a][3 + a] = 1.0;
      o.res[3 + a] = u.zp[j][a] - (u.p[a] + pred[a]);
    }
  }
  for (int k = 0; k < kChainMaxRows * kChainMaxRows; k++) o.R[k] = u.R[j][k];
  for (int k = 0; k < kChainMaxCols; k++)
    o.hidx[k] = k < 6              ? u.id_imu + k
                : (arm && k < 9) ? u.id_arm[j] + k - c_arm
                : (rot && k < n) ? u.id_rot[j] + k - c_rot
                                 : 0;
  o.thr = u.thr[j];
  o.n = n;
  o.pad = 0;
  chain_reset(region, halt);
}

void launch_pose_rows(hipStream_t s, DPoseState *st, int j, const DChainRegion *prev, DChainRow *row,
                      DChainRegion *region) {
  hipLaunchKernelGGL(k_pose_rows, dim3(1), dim3(64), 0, s, st, j, prev, row, region);
}

template <int R>
__global__ void __launch_bounds__(256) k_chain_M(const double *__restrict__ P, int ldp, int N,
                                                 const DChainRow *__restrict__ row, double *__restrict__ M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double *Pr = P + (size_t)i * ldp;
  const int n = row->n;
  double a[R];
#pragma unroll
  for (int c = 0; c < R; c++) a[c] = 0.0;
  for (int k = 0; k < n; k++) {
    const double pv = Pr[row->hidx[k]];
#pragma unroll
    for (int c = 0; c < R; c++) a[c] = fma(pv, row->H[c][k], a[c]);
  }
#pragma unroll
  for (int c = 0; c < R; c++) M[(size_t)c * N + i] = a[c];
}

void launch_chain_M(hipStream_t s, const double *P, int ldp, int N, const DChainRow *row, int r, double *M) {
  if (r != 1 && r != 2 && r != 3 && r != 6) throw std::runtime_error("measurement chain: " + std::to_string(r) + " rows");
  auto *k = r == 1 ? k_chain_M<1> : r == 2 ? k_chain_M<2> : r == 3 ? k_chain_M<3> : k_chain_M<kChainMaxRows>;
  hipLaunchKernelGGL(k, dim3((N + 255) / 256), dim3(256), 0, s, P, ldp, N, row, M);
}

// The two gate policies of k_chain_update: from S, what the header gets and whether the step is applied; then the
// weights w of a row m of M with P[i][j] -= ww(w_i, w_j) and dx[j] = dx(w_j).  They are NOT one policy at R = 1:
// the range gate lets a NaN chi2 (and a negative S) through as the reference does and divides by sqrt(S) once,
// the fix gate refuses both and substitutes through its Cholesky factor.  Routing a range through the factor, or
// making its gate refuse NaN, changes results.
struct RangeGate {  // UpdaterUWB.cpp:73-79: rejected when chi2 > multiplier * chi2_0.95(1)
  static constexpr int R = 1;
  double res, rs;
  __device__ bool gate(const double (&S)[1][1], const DChainRow &row, double &chi2, double &extra) {
    res = row.res[0];
    chi2 = res * res / S[0][0];
    extra = S[0][0];
    rs = 1.0 / sqrt(S[0][0]);
    return !(chi2 > row.thr);
  }
  __device__ void weights(const double *m, int, double (&w)[1]) const { w[0] = m[0] * rs; }
  __device__ double ww(const double (&wi)[1], const double (&wj)[1]) const { return wi[0] * wj[0]; }
  __device__ double dx(const double (&wj)[1]) const { return wj[0] * (res * rs); }
};
template <int R_>
struct FixGate {  // S = L L^T in registers, y = L^-1 res, chi2 = |y|^2
  static constexpr int R = R_;
  double L[R][R], y[R];
  __device__ bool gate(const double (&S)[R][R], const DChainRow &row, double &chi2_out, double &extra) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < R; j++) {
      double d = S[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
      if (!(isfinite(d) && d > 0.0)) bad = true;
      L[j][j] = sqrt(d);
#pragma unroll
      for (int i = j + 1; i < R; i++) {
        double v = S[j][i];
#pragma unroll
        for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
        L[i][j] = v / L[j][j];
      }
    }
    double chi2 = 0.0;
#pragma unroll
    for (int i = 0; i < R; i++) {
      double v = row.res[i];
#pragma unroll
      for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
      y[i] = v / L[i][i];
      chi2 += y[i] * y[i];
    }
    const bool refused = bad || chi2 != chi2;
    chi2_out = bad ? __builtin_nan("") : chi2;
    extra = refused ? 1.0 : 0.0;
    return !refused && !(chi2 > row.thr);
  }
  // a row of W = M L^-T: L w^T = m^T by forward substitution
  __device__ void weights(const double *m, int N, double (&w)[R]) const {
#pragma unroll
    for (int c = 0; c < R; c++) {
      double v = m[(size_t)c * N];
#pragma unroll
      for (int k = 0; k < c; k++) v -= L[c][k] * w[k];
      w[c] = v / L[c][c];
    }
  }
  __device__ double ww(const double (&wi)[R], const double (&wj)[R]) const {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < R; c++) s += wi[c] * wj[c];
    return s;
  }
  __device__ double dx(const double (&wj)[R]) const {
    double d = 0.0;
#pragma unroll
    for (int c = 0; c < R; c++) d += wj[c] * y[c];
    return d;
  }
};

// tile pair (bi, bj), bi <= bj, of the 16 x 16 tiles of P, one element per thread
template <class G>
__global__ void __launch_bounds__(256) k_chain_update(double *__restrict__ P, int ldp, int N,
                                                      const double *__restrict__ M,
                                                      const DChainRow *__restrict__ row,
                                                      DChainRegion *__restrict__ region, int nb) {
  if (region->halt != 0) return;  // halted (the row kernel): not applied, accepted stays 0
  // the innovation covariance and the gate, the same arithmetic in every block
  constexpr int R = G::R;
  const int n = row->n;
  double S[R][R];
#pragma unroll
  for (int a = 0; a < R; a++)
#pragma unroll
    for (int b = a; b < R; b++) {
      double acc = 0.0;
      for (int k = 0; k < n; k++) acc = fma(row->H[a][k], M[(size_t)b * N + row->hidx[k]], acc);
      S[a][b] = acc + row->R[kChainMaxRows * a + b];
    }
  G g;
  double chi2, extra;
  const bool acc = g.gate(S, *row, chi2, extra);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    region->accepted = acc ? 1.0 : 0.0;
    region->chi2 = chi2;
    region->extra = extra;
  }
  if (!acc) return;
  int bi, bj;
  upper_pair(blockIdx.x, nb, bi, bj);
  const int ei = threadIdx.x >> 4, ej = threadIdx.x & 15;
  const int gi = 16 * bi + ei, gj = 16 * bj + ej;
  if (gi >= N || gj >= N) return;
  double wi[R], wj[R];
  g.weights(M + gi, N, wi);
  g.weights(M + gj, N, wj);
  if (bi < bj || ej >= ei) {
    const double v = P[(size_t)gi * ldp + gj] - g.ww(wi, wj);
    P[(size_t)gi * ldp + gj] = v;
    P[(size_t)gj * ldp + gi] = v;
    if (gi == gj && v < 0.0) atomicAdd(&region->neg, 1);
  }
  if (bi == bj && ei == 0) region->dx[gj] = g.dx(wj);
}

void launch_chain_update(hipStream_t s, double *P, int ldp, int N, const double *M, const DChainRow *row, int r,
                         bool range, DChainRegion *region) {
  if ((r != 1 && r != 2 && r != 3 && r != 6) || (range && r != 1))
    throw std::runtime_error("measurement chain: " + std::to_string(r) + " rows");
  const int nb = (N + 15) / 16;
  auto *k = range    ? k_chain_update<RangeGate>
            : r == 1 ? k_chain_update<FixGate<1>>
            : r == 2 ? k_chain_update<FixGate<2>>
            : r == 3 ? k_chain_update<FixGate<3>>
                     : k_chain_update<FixGate<kChainMaxRows>>;
  hipLaunchKernelGGL(k, dim3(nb * (nb + 1) / 2), dim3(256), 0, s, P, ldp, N, M, row, region, nb);
}

static void ensure_ekf_lds_attrs() {
  static bool done = false;
  if (done) return;
  const void *fns[12] = {(const void *)k_ekf_MS,
                         (const void *)k_ekf_WP,
                         (const void *)k_ekf_fact<1, true, false>,
                         (const void *)k_ekf_fact<2, true, false>,
                         (const void *)k_ekf_fact<3, true, false>,
                         (const void *)k_ekf_fact<4, true, false>,
                         (const void *)k_ekf_fact<5, true, false>,
                         (const void *)k_ekf_fact<1, true, true>,
                         (const void *)k_ekf_fact<2, true, true>,
                         (const void *)k_ekf_fact<3, true, true>,
                         (const void *)k_ekf_fact<4, true, true>,
                         (const void *)k_ekf_fact<5, true, true>};
  for (int k = 0; k < 12; k++)
    if (set_dyn_lds(fns[k], kMaxDynLds) < kMaxDynLds)
      throw std::runtime_error("dynamic LDS limit not granted for an EKF kernel (" + std::to_string(k) + ")");
  done = true;
}

void launch_ekf_phaseA(hipStream_t s, const double *P, int ldp, int N, const double *H, int ldh, int r, int n,
                       const int *hidx, double sigma2, EkfScratch &sc) {
  ensure_ekf_lds_attrs();
  const size_t lds = ekf_ms_lds_bytes(n);
  if (lds > (size_t)kMaxDynLds) throw std::runtime_error("EKF update with too many columns for k_ekf_MS");
  const int nbM = (N + 15) / 16, nt = (r + 15) / 16;
  const int wpb = kMSThreads / 64;
  const int nbS = (nt * (nt + 1) / 2 + wpb - 1) / wpb;  // the upper tile pairs, a wave each
  double *Sup = sc.S + 2 * (size_t)r * r;
  if (!sc.Tall) {
    // No T from a chi2 gate: S from this update's own M in a second launch (rows hidx of M are T^T)
    hipLaunchKernelGGL(k_ekf_MS, dim3(nbM), dim3(kMSThreads), lds, s, P, ldp, N, H, ldh, r, n, hidx, sigma2, sc.M, Sup,
                       nbM, sc.neg, (const double *)nullptr, 0, (const unsigned long long *)nullptr);
    hipLaunchKernelGGL(k_ekf_MS, dim3(nbS), dim3(kMSThreads), lds, s, P, ldp, N, H, ldh, r, n, hidx, sigma2, sc.M, Sup,
                       0, (int *)nullptr, (const double *)sc.M, -1, (const unsigned long long *)nullptr);
    return;
  }
  hipLaunchKernelGGL(k_ekf_MS, dim3(nbM + nbS), dim3(kMSThreads), lds, s, P, ldp, N, H, ldh, r, n, hidx, sigma2, sc.M, Sup,
                     nbM, sc.neg, sc.Tall, sc.ldt, sc.kmask_tile);
}

template <bool LDS, bool DENSE_R>
static auto ekf_fact_instance(int w) {
  return w == 1   ? k_ekf_fact<1, LDS, DENSE_R>
         : w == 2 ? k_ekf_fact<2, LDS, DENSE_R>
         : w == 3 ? k_ekf_fact<3, LDS, DENSE_R>
         : w == 4 ? k_ekf_fact<4, LDS, DENSE_R>
                  : k_ekf_fact<5, LDS, DENSE_R>;
}

// k_ekf_fact on sc.S's S_up (+ R when R is given: the dense gate against chi2_thr into sc.chi2_gate, else the
// plain gate of sc.chi2_gate / sc.chi2_thr when the scratch has one)
static void launch_ekf_factor(hipStream_t s, int N, int r, const double *res, int res_stride, EkfScratch &sc,
                              const double *R = nullptr, int ldr = 0, double chi2_thr = 0.0) {
  ensure_ekf_lds_attrs();
  if (r + 1 > kWaveMaxRows) throw std::runtime_error("direct EKF update with more rows than the factorization panel");
  const size_t bytes = ekf_small_lds_bytes(r);
  const bool use_lds = bytes <= (size_t)kMaxDynLds;
  double *Linv = sc.S;
  double *Sup = sc.S + 2 * (size_t)r * r;
  double *Sg = sc.S + 3 * (size_t)r * r;  // (r+1)(r|1) + 2r <= 2 r^2 doubles once r >= 40 (else LDS)
  {
    KScope ks(sc.kp, KC_LDL);
    const int w = panel_waves(r + 1);
    auto *kf = R ? (use_lds ? ekf_fact_instance<true, true>(w) : ekf_fact_instance<false, true>(w))
                 : (use_lds ? ekf_fact_instance<true, false>(w) : ekf_fact_instance<false, false>(w));
    hipLaunchKernelGGL(kf, dim3(1), dim3(kFactThreads), use_lds ? bytes : 0, s, Sup, r, R, ldr, res, res_stride, Linv,
                       sc.y, Sg, sc.chi2_gate, R ? chi2_thr : sc.chi2_thr, sc.dx + N);
  }
  // LDL^T of the r x r innovation covariance with the residual as an extra row: r^3/3 + r^2 FLOPs; the
  // lower triangle (and R's) and the residual read, the factor written
  if (sc.kp) sc.kp->credit(KC_LDL, (double)r * r * r / 3.0 + (double)r * r, 8.0 * ((R ? 2.0 : 1.5) * r * r + 2.0 * r));
  if (sc.chi2_gate) sc.gate = sc.chi2_gate;
}

// k_ekf_WP over the upper tile pairs of P with the factor launch_ekf_factor left in sc
static void launch_ekf_WP(hipStream_t s, double *P, int ldp, int N, int r, EkfScratch &sc, const int *gate) {
  const int nb = (N + 15) / 16;
  const size_t lw = (size_t)(32 * (r | 1) + 1024) * sizeof(double);
  hipLaunchKernelGGL(k_ekf_WP, dim3(nb * (nb + 1) / 2), dim3(256), lw, s, P, ldp, N, sc.M, r, sc.S, sc.y, sc.dx,
                     sc.neg, gate, nb);
}

void launch_ekf_phaseB(hipStream_t s, double *P, int ldp, int N, int r, const double *res, int res_stride,
                       EkfScratch &sc) {
  launch_ekf_factor(s, N, r, res, res_stride, sc);
  launch_ekf_WP(s, P, ldp, N, r, sc, sc.gate);
}

// ---------------------------------------------------------------------------------------------------
// One delayed-initialization candidate (StateHelper::initialize, StateHelper.cpp:393-577: initialize_invertible
// of the landmark's 3 rows, then EKFUpdate of the other nup rows at the same factor that carries the chi2 test)
// in six launches, the linearization (k_feature) before these five included; H holds the landmark's D
// initializing rows H_init, then the nup update rows H_up:
//   k_di_M    grid over the old state's 16-row blocks (rows < Ni), P[i, I] staged once in LDS:
//             M_up = P[:, I] H_up^T (Ni x nup) on 16x16 MFMA tiles, one column tile per wave, ascending k;
//             M3 = P[:, I] H_init^T (Ni x D) as a GEMV: one wavefront per row, lanes over the columns k (stride
//             64, fma in ascending k), then a butterfly sum over the lanes (xor 32, 16, .. 1)
//   k_di_S    three kinds of block:
//             [0, nbG)        S_up = H_up T^T + s2 I with T^T = M_up's rows I: one upper tile pair per wave
//             [nbG, nbG+nbX)  initialize_invertible: the landmark's cross-covariance columns -M3 H_Linv^T, 512
//                             elements per block; the first block also its D x D block H_Linv (H_init M3[I] +
//                             s2 I) H_Linv^T, each element of H_init M3[I] as 28 strided partials (k = j, j + 28,
//                             ..) added in the fixed order j = 0 .. 27
//             the last        the landmark's rows Ni .. Ni+D-1 of M_up: P's new rows recomputed from M3 by the
//                             expression the blocks before it store, then the MFMA tiles of k_di_M
//   k_ekf_fact, k_ekf_WP, k_chain_apply as in every other update
// The arithmetic is StateHelper::initialize_invertible's and EKFUpdate's; these summation orders fix every bit of
// the result (the 40-frame state digests of cfg3 and cfg3t), so they are not to be changed.
// Measured and dropped: k_chain_apply folded into k_ekf_WP (the last workgroup to finish, after agent-scope
// release / acquire fences around a completion counter, moving the tables): 22.8 us against 10.7 + 4.7 us.
template <int D>
__global__ void __launch_bounds__(kMSThreads) k_di_M(const double *__restrict__ P, int ldp, int Ni,
                                              const double *__restrict__ H, int ldh, int nup, int n,
                                              const int *__restrict__ hidx, double *__restrict__ M,
                                              double *__restrict__ M3, int *neg) {
  extern __shared__ double sh[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  if (blockIdx.x == 0 && threadIdx.x == 0) *neg = 0;  // the update's negative-diagonal count
  const int i0 = blockIdx.x * 16, lds = n | 1;
  double *Ps = sh;
  staged_copy(
      16 * n,
      [&](int e) {
        const int i = e / n, k = e - i * n;
        return (i0 + i < Ni) ? P[(size_t)(i0 + i) * ldp + hidx[k]] : 0.0;
      },
      [&](int e, double v) {
        const int i = e / n, k = e - i * n;
        Ps[i * lds + k] = v;
      });
  __syncthreads();
  const double *Hup = H + D * (size_t)ldh;
  const int nct = (nup + 15) / 16;
  for (int t = wid; t < nct; t += kMSThreads / 64) {
    const int j0 = 16 * t, jr = j0 + r16;
    const double *Hr = Hup + (size_t)min(jr, nup - 1) * ldh;
    const bool jv = jr < nup;
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = tile_chain<16>(
        0, n, kq, [&](int k) { return Ps[r16 * lds + k]; }, [&](int k) { return jv ? Hr[k] : 0.0; }, acc);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = i0 + kq + 4 * q, col = j0 + r16;
      if (row < Ni && col < nup) M[(size_t)row * nup + col] = acc[q];
    }
  }
  // M3: one wavefront per row, lanes over the columns, butterfly sum
  for (int i = wid; i < 16 && i0 + i < Ni; i += kMSThreads / 64) {
    double acc[kSmallMRows] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < n; k += 64) {
      const double p = Ps[i * lds + k];
#pragma unroll
      for (int b = 0; b < D; b++) acc[b] = fma(p, H[(size_t)b * ldh + k], acc[b]);
    }
#pragma unroll
    for (int b = 0; b < kSmallMRows; b++)
      for (int o = 32; o > 0; o >>= 1) acc[b] += __shfl_xor(acc[b], o, 64);
    if (lane < D) {
      double v = acc[0];
#pragma unroll
      for (int b = 1; b < kSmallMRows; b++)
        if (lane == b) v = acc[b];
      M3[(size_t)(i0 + i) * D + lane] = v;
    }
  }
}

constexpr int kDiInitThreads = 512;  // k_di_S's initialize_invertible blocks: (D Ni + 511) / 512 of them
// H_Linv of the landmark's D x D H_finit (DFeatOut::HfR): the host's cofactor formula, or the scalar's reciprocal
template <int D>
__device__ __forceinline__ void di_hinv(const double *HfR, double *Hinv) {
  if (D == 3)
    inv3_cofactor(HfR, Hinv);
  else
    Hinv[0] = 1.0 / HfR[0];
}
template <int D>
__global__ void __launch_bounds__(kMSThreads) k_di_S(double *__restrict__ P, int ldp, int Ni,
                                              const double *__restrict__ H, int ldh, int nup, int n,
                                              const int *__restrict__ hidx, double s2, double *__restrict__ M,
                                              const double *__restrict__ M3, double *__restrict__ Sup,
                                              const DFeatOut *__restrict__ fout, const int *__restrict__ gate,
                                              double *__restrict__ resout, int nbG, int nbX) {
  extern __shared__ double sh[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const double *Hup = H + D * (size_t)ldh;
  const int b = blockIdx.x;
  if (b < nbG) {
    // S_up[a][b] = H_a T_b^T with T[b][k] = M[hidx[k]][b] (as k_ekf_MS with ldt < 0)
    int *hs = (int *)sh;
    for (int k = threadIdx.x; k < n; k += blockDim.x) hs[k] = hidx[k];
    __syncthreads();
    const int nt = (nup + 15) / 16;
    const int pair = b * (kMSThreads / 64) + wid;
    if (pair >= nt * (nt + 1) / 2) return;
    int at, bt;
    upper_pair(pair, nt, at, bt);
    const int ar = 16 * at + r16, br = 16 * bt + r16;
    const double *Ha = Hup + (size_t)min(ar, nup - 1) * ldh;
    const double *Tb = M + min(br, nup - 1);
    const bool av = ar < nup, bv = br < nup;
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = tile_chain<16>(
        0, n, kq, [&](int k) { return av ? Ha[k] : 0.0; }, [&](int k) { return bv ? Tb[(size_t)hs[k] * nup] : 0.0; },
        acc);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = 16 * at + kq + 4 * q, col = 16 * bt + r16;
      if (row < nup && col < nup) Sup[(size_t)row * nup + col] = acc[q] + (row == col ? s2 : 0.0);
    }
    return;
  }
  constexpr int DD = D * D;
  __shared__ double Hinv[DD], S3[DD], PLL[DD];
  if (b < nbG + nbX) {
    // initialize_invertible: block xb takes the cross-covariance elements xb * 512 ..; the first one also the
    // D x D block
    const int xb = b - nbG, t = threadIdx.x + xb * kDiInitThreads;
    if (resout && xb == 0 && threadIdx.x < D) resout[threadIdx.x] = H[(size_t)threadIdx.x * ldh + n];
    if (gate && *gate == 0) return;
    if (threadIdx.x == 0) di_hinv<D>(fout->HfR, Hinv);
    __syncthreads();
    if (xb == 0) {
      __shared__ double part[DD][28];
      const int e = threadIdx.x / 28, j = threadIdx.x % 28;
      if (e < DD) {
        const int a = e / D, bb = e % D;
        double acc = 0.0;
        for (int k = j; k < n; k += 28) acc += H[(size_t)a * ldh + k] * M3[(size_t)hidx[k] * D + bb];
        part[e][j] = acc;
      }
      __syncthreads();
      if (threadIdx.x < DD) {
        const int a = threadIdx.x / D, bb = threadIdx.x % D;
        double acc = 0.0;
        for (int q = 0; q < 28; q++) acc += part[threadIdx.x][q];
        S3[threadIdx.x] = acc + (a == bb ? s2 : 0.0);
      }
      __syncthreads();
      if (threadIdx.x < DD) {
        const int a = threadIdx.x / D, bb = threadIdx.x % D;
        double acc = 0.0;
        for (int c = 0; c < D; c++)
          for (int e2 = 0; e2 < D; e2++) {
            const double sce = (c <= e2) ? S3[c * D + e2] : S3[e2 * D + c];
            acc += Hinv[a * D + c] * sce * Hinv[bb * D + e2];
          }
        PLL[threadIdx.x] = acc;
      }
    }
    if (t < Ni * D) {
      const int i = t / D, a = t % D;
      double acc = 0.0;
      for (int bb = 0; bb < D; bb++) acc += M3[(size_t)i * D + bb] * Hinv[a * D + bb];
      P[(size_t)i * ldp + Ni + a] = -acc;
      P[(size_t)(Ni + a) * ldp + i] = -acc;
    }
    if (xb == 0 && threadIdx.x < DD) {
      const int a = threadIdx.x / D, bb = threadIdx.x % D;
      P[(size_t)(Ni + a) * ldp + Ni + bb] = PLL[threadIdx.x];
    }
    return;
  }
  // the landmark's rows Ni .. Ni+D-1 of M_up: P[Ni + a][hidx[k]] as initialize_invertible writes it, then the
  // 16-row tiles of k_ekf_MS (only these D rows of the tile are stored)
  if (gate && *gate == 0) return;
  double *Pl = sh;  // D x n
  if (threadIdx.x == 0) di_hinv<D>(fout->HfR, Hinv);
  __syncthreads();
  for (int e = threadIdx.x; e < D * n; e += blockDim.x) {
    const int a = e / n, k = e - a * n, i = hidx[k];
    double acc = 0.0;
    for (int bb = 0; bb < D; bb++) acc += M3[(size_t)i * D + bb] * Hinv[a * D + bb];
    Pl[e] = -acc;
  }
  __syncthreads();
  const int nct = (nup + 15) / 16;
  for (int t = wid; t < nct; t += kMSThreads / 64) {
    const int j0 = 16 * t, jr = j0 + r16;
    const double *Hr = Hup + (size_t)min(jr, nup - 1) * ldh;
    const bool jv = jr < nup, rv = r16 < D;
    dbl4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = tile_chain<16>(
        0, n, kq, [&](int k) { return rv ? Pl[r16 * n + k] : 0.0; }, [&](int k) { return jv ? Hr[k] : 0.0; }, acc);
    const int col = j0 + r16;
    if (kq < D && col < nup) M[(size_t)(Ni + kq) * nup + col] = acc[0];
  }
}

template <int D>
static void di_candidate(hipStream_t s, double *P, int ldp, int Ni, const double *Hrow, int ldh, int nup, int n,
                         const int *hidx, double s2, EkfScratch &sc, const DFeatOut *fout, double *resout,
                         DClone *clones, DPoseVal *cv, int ncl, DCam *cams, DPoseVal *camv, int ncam, int calib_ext,
                         int calib_intr, double *out) {
  if (nup <= 0 || nup + 1 > kWaveMaxRows) throw std::runtime_error("delayed-init candidate rows outside 1..255");
  if (ncl + ncam > 256) throw std::runtime_error("update chain: more clones + cameras than one workgroup");
  if (!sc.M3 || !sc.chi2_gate) throw std::runtime_error("delayed-init candidate: scratch not set up");
  ensure_ekf_lds_attrs();
  static bool attrs = false;
  if (!attrs) {
    if (set_dyn_lds((const void *)k_di_M<D>, kMaxDynLds) < kMaxDynLds ||
        set_dyn_lds((const void *)k_di_S<D>, kMaxDynLds) < kMaxDynLds)
      throw std::runtime_error("dynamic LDS limit not granted for a delayed-init kernel");
    attrs = true;
  }
  const size_t ldsM = (size_t)16 * (n | 1) * sizeof(double);
  const size_t ldsS = std::max((size_t)n * sizeof(int), (size_t)D * n * sizeof(double));
  if (ldsM > (size_t)kMaxDynLds || ldsS > (size_t)kMaxDynLds)
    throw std::runtime_error("delayed-init candidate with too many columns");
  const int N = Ni + D;
  {
    hipLaunchKernelGGL(k_di_M<D>, dim3((Ni + 15) / 16), dim3(kMSThreads), ldsM, s, P, ldp, Ni, Hrow, ldh, nup, n, hidx,
                       sc.M, sc.M3, sc.neg);
    const int nt = (nup + 15) / 16, wpb = kMSThreads / 64;
    const int nbG = (nt * (nt + 1) / 2 + wpb - 1) / wpb, nbX = (D * Ni + kDiInitThreads - 1) / kDiInitThreads;
    double *Sup = sc.S + 2 * (size_t)nup * nup;
    hipLaunchKernelGGL(k_di_S<D>, dim3(nbG + nbX + 1), dim3(kMSThreads), ldsS, s, P, ldp, Ni, Hrow, ldh, nup, n, hidx,
                       s2, sc.M, sc.M3, Sup, fout, sc.chi2_gate, resout, nbG, nbX);
    launch_ekf_factor(s, N, nup, Hrow + D * (size_t)ldh + n, ldh, sc);
    launch_ekf_WP(s, P, ldp, N, nup, sc, sc.chi2_gate);
  }
  launch_chain_apply(s, fout, sc.chi2_gate, sc.neg, sc.dx, clones, cv, ncl, cams, camv, ncam, calib_ext, calib_intr,
                     nullptr, 0, P, ldp, N, Ni, out, D);
}

void launch_di_candidate(hipStream_t s, double *P, int ldp, int Ni, const double *Hrow, int ldh, int nup, int n,
                         const int *hidx, double s2, EkfScratch &sc, const DFeatOut *fout, double *resout,
                         DClone *clones, DPoseVal *cv, int ncl, DCam *cams, DPoseVal *camv, int ncam, int calib_ext,
                         int calib_intr, double *out, int d) {
  if (d == 3)
    di_candidate<3>(s, P, ldp, Ni, Hrow, ldh, nup, n, hidx, s2, sc, fout, resout, clones, cv, ncl, cams, camv, ncam,
                    calib_ext, calib_intr, out);
  else if (d == 1)
    di_candidate<1>(s, P, ldp, Ni, Hrow, ldh, nup, n, hidx, s2, sc, fout, resout, clones, cv, ncl, cams, camv, ncam,
                    calib_ext, calib_intr, out);
  else
    throw std::runtime_error("delayed-init candidate: landmark dimension " + std::to_string(d));
}

void launch_ekf_update(hipStream_t s, double *P, int ldp, int N, const double *H, int ldh, int r, int n,
                       const int *hidx, const double *res, int res_stride, double sigma2, EkfScratch &sc) {
  launch_ekf_phaseA(s, P, ldp, N, H, ldh, r, n, hidx, sigma2, sc);
  launch_ekf_phaseB(s, P, ldp, N, r, res, res_stride, sc);
}

// StateHelper::EKFUpdate (StateHelper.cpp:116-197) with the caller's dense R behind a chi2 gate on its own factor
// (UpdaterUWB.cpp:67-79): phase A with s2 = 0, k_ekf_fact's dense-R instance, k_ekf_WP behind the gate int
// sc.chi2_gate.  As many launches as launch_ekf_update; M, the factor and the P update are that path's kernels.
void launch_ekf_update_R(hipStream_t s, double *P, int ldp, int N, const double *H, int ldh, int r, int n,
                         const int *hidx, const double *res, int res_stride, const double *R, int ldr, double chi2_thr,
                         EkfScratch &sc) {
  if (!sc.chi2_gate) throw std::runtime_error("EKF update with R: no gate in the scratch");
  if (!R) throw std::runtime_error("EKF update with R: no R");
  if (r + 1 > kWaveMaxRows) throw std::runtime_error("direct EKF update with more rows than the factorization panel");
  if (ldr < r) throw std::runtime_error("EKF update: leading dimension of R below its row count");
  if (sc.Tall) throw std::runtime_error("EKF update with R: T of another H in the scratch");
  launch_ekf_phaseA(s, P, ldp, N, H, ldh, r, n, hidx, 0.0, sc);
  launch_ekf_factor(s, N, r, res, res_stride, sc, R, ldr, chi2_thr);
  launch_ekf_WP(s, P, ldp, N, r, sc, sc.chi2_gate);
}

}  // namespace uvhp
