// rl_global2_kernel.hpp -- the body of k_global_qp2, included TWICE by rl_global2.hpp (no include guard): with RL_G2_WEIGHTED 0
// it is k_global_qp2, token for token the kernel it always was (so are its registers and spills), with RL_G2_WEIGHTED 1 it is
// k_global_qp2_weighted.  Everything the two share is written once, here.

// ------------------------------------------------------------------------------------------------
// Barrier protocol.  Both roles execute exactly this sequence (R = row waves, L = linear-algebra wave):
//
//   per outer iteration
//     [Oa] all: control points from the offsets                                  -> barrier
//     [Ob] R: curvature rows, Gauss-Newton partials (27 outputs)                 -> flush (3 rounds:
//          R writes Spart | barrier | all reduce | barrier)    -- the first barrier also publishes
//          sum kappa^2; every thread leaves the outer loop here when outer == n_outer
//     [Oc] L: P, q (scaled), x = a.   R: lo/hi, initial slacks and duals         -> barrier
//     per interior-point iteration
//       [I1] R: residuals, A'DA / A'e / A'(lu-ll) partials (33 outputs).  L: P x + q   -> flush (3 rounds)
//       [I2] all: folded normal matrix, rd, rhs                                   -> barrier
//       [I3] L: convergence test -> ctl[0]; factor; affine solve -> dxs          -> barrier
//            all: leave the loop when ctl[0] != 0
//       [I4] R: affine step: ratios, complementarity sums -> red; corrector partials A'w0 and
//            A'(1/sl - 1/su) (2(K+1) outputs) -> Spart                            -> barrier
//       [I5] all: reduce                                                          -> barrier
//       [I6] L: alpha_aff, sigma -> ctl[1]; second right-hand side; solve -> dxs -> barrier
//       [I7] R: step ratios -> red                                                -> barrier
//       [I8] all: alpha.  R: update slacks/duals.  L: x += alpha dx              -> barrier
//     [Od] L: a = x, step size                                                   -> barrier
//
// RL_G2_WEIGHTED (k_global_qp2_weighted): the cost is sum_i w[b][i] kappa_i^2, weights [B][N], sample i of instance b as the SPEED
// column of that instance's table.  The weight enters in [Ob] alone -- one global load per row, then w kappa^2, w G'G and
// w G'(kappa - G a) -- so LDS, barriers and the linear-algebra wave are those of the unweighted kernel.  The products are
// (G w) G, (G w) res and (kappa w) kappa: w = 1 multiplies by one (the unweighted kernel's values operation for operation),
// and a constant power of two scales every partial exactly, which the trace scaling sc = np / tr cancels (a, ctrl and xy
// keep the bits of w = 1; stats[1], stats[2] are the exact multiple).  The kernel validates its own weights: in the prologue
// every thread counts those outside [kWeightMin, kWeightMax] (NaN fails), the per-wave counts travel through `red` with the
// prologue's own barrier, and every thread sums them BEFORE the role split: the verdict is workgroup-uniform and the
// barrier protocol that follows is the same for every thread.  A refused instance runs as n_outer = 0 (its outputs are the
// input line; stats[1], stats[2] unspecified) and reports the number of refused weights in stats[6].
#if RL_G2_WEIGHTED
#define RL_G2_N_OUTER n_outer
template <int K, int R, int G, bool AREG>
__global__ void __launch_bounds__(kG2Block) k_global_qp2_weighted(GlobalArgs a, const double* __restrict__ weights) {
#else
#define RL_G2_N_OUTER a.n_outer
template <int K, int R, int G, bool AREG>
__global__ void __launch_bounds__(kG2Block) k_global_qp2(GlobalArgs a) {
#endif
  constexpr int K1 = K + 1, NE = K1 * (K1 + 1) / 2, NO = NE + 2 * K1, BW = 2 * K, GR = g2_round(G);
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int nt = blockDim.x, nrw = (nt >> 6) - 1, nrow = nrw * kWave;
  const bool la = wave == nrw;
  const int b = blockIdx.x;
  const int N = a.trk.N, n = a.trk.n, np = a.np;
  const Global2Layout L = global2_layout(K, n, np, N, G, nrow);
  double *xsA = lds + L.xs, *xsB = lds + L.xs2, *dxa = lds + L.dxa, *dxs = lds + L.dxs, *avs = lds + L.avs, *qv = lds + L.qv, *rdP = lds + L.rdP;
  double *rd = lds + L.rd, *rhs = lds + L.rhs, *cxs = lds + L.cxs, *cys = lds + L.cys, *nus = lds + L.nus;
  double *Pc = lds + L.Pc, *band = lds + L.band, *Ssum = lds + L.Ssum, *Spart = lds + L.Spart, *Mf = lds + L.Spart;
  short* itab = reinterpret_cast<short*>(lds + L.itab);
  double *lohi = lds + L.lohi, *red = lds + L.red, *ctl = lds + L.ctl;
  int* sch = reinterpret_cast<int*>(lds + L.sch);
  const double* __restrict__ wid = a.widths + (size_t)b * N * 2;

  for (int j = tid; j < np; j += nt) { nus[2 * j] = a.nu[2 * j]; nus[2 * j + 1] = a.nu[2 * j + 1]; avs[j] = 0.0; }
  for (int j = tid; j <= np; j += nt) sch[j] = a.span_ch0[j];
  if constexpr (G == 1) TwoFront<BW>::build_index_table(tid, nt, np, itab);
  for (int i = tid; i < N; i += nt) {
    const double2 w = reinterpret_cast<const double2*>(wid)[i];
    reinterpret_cast<double2*>(lohi)[i] = make_double2(-(w.y - a.margin), w.x - a.margin);
  }
#if RL_G2_WEIGHTED
  const double* __restrict__ wrow = weights + (size_t)b * N;
  {
    double bad = 0.0;
    for (int i = tid; i < N; i += nt) {
      const double w = wrow[i];
      if (!(w >= kWeightMin && w <= kWeightMax)) bad += 1.0;   // NaN fails both comparisons
    }
    bad = wave_sum(bad);
    if (lane == 0) red[48 + wave] = bad;   // the fourth block of `red`: nothing else uses it
  }
#endif
  __syncthreads();
#if RL_G2_WEIGHTED
  double refused = 0.0;   // workgroup-uniform: every thread adds the same counts in the same order
  for (int w = 0; w <= nrw; ++w) refused += red[48 + w];
  const int n_outer = __builtin_amdgcn_readfirstlane(refused != 0.0 ? 0 : a.n_outer);   // scalar, as a.n_outer is
#endif

  // block-level combine of the row waves' partials (fixed order)
  auto red_sum = [&](int kind) { double s = 0.0; for (int w = 0; w < nrw; ++w) s += red[kind * 16 + w]; return s; };
  auto red_max = [&](int kind) { double s = -INFINITY; for (int w = 0; w < nrw; ++w) s = fmax(s, red[kind * 16 + w]); return s; };
  double k2_first = 0.0, k2_last = 0.0;
  int total_it = 0;

  if (!la) {
    // =================================================================================== row waves
    const bool has = tid < a.nc;
    int row0 = 0, cnt = 0, sp0 = 0;
    if (has) {
      const int2 c = reinterpret_cast<const int2*>(a.chunk)[tid];
      row0 = c.x & 0xffffff; cnt = (unsigned)c.x >> 24; sp0 = c.y;
    }
    int J[K1];
#pragma unroll
    for (int al = 0; al < K1; ++al) { J[al] = sp0 + al; if (J[al] >= np) J[al] -= np; }
    ChunkRows<K1, R, AREG> rows;
    const double* __restrict__ D1 = a.trk.D + (size_t)K1 * N;
    const double* __restrict__ D2 = a.trk.D + (size_t)2 * K1 * N;
    double sl[R] = {}, su[R] = {}, ll[R] = {}, lu[R] = {};
#ifdef RL_G2_PROFILE
    long long rT[6] = {0, 0, 0, 0, 0, 0}, rk = wall_clock64();
#define G2_LAP(i) { const long long n_ = wall_clock64(); rT[i] += n_ - rk; rk = n_; }
#else
#define G2_LAP(i)
#endif

    for (int outer = 0;; ++outer) {
      // [Oa]
      for (int j = tid; j < n; j += nt) {
        const int jj = j >= np ? j - np : j;
        cxs[j] = fma(avs[jj], nus[2 * jj], a.trk.c0[jj]);
        cys[j] = fma(avs[jj], nus[2 * jj + 1], a.trk.c0[n + jj]);
      }
      __syncthreads();
      // [Ob]
      {
        double acc[NE + K1];
#pragma unroll
        for (int o = 0; o < NE + K1; ++o) acc[o] = 0.0;
        double k2p = 0.0;
        if (has) {
          double cxJ[K1], cyJ[K1];
#pragma unroll
          for (int al = 0; al < K1; ++al) { cxJ[al] = cxs[sp0 + al]; cyJ[al] = cys[sp0 + al]; }
#pragma unroll 1
          for (int r = 0; r < cnt; ++r) {
            const int i = row0 + r;
#if RL_G2_WEIGHTED
            const double wi = wrow[i];   // the one load of the weight, in flight with the basis rows
#endif
            double b1[K1], b2[K1], dx = 0, dy = 0, ddx = 0, ddy = 0;
#pragma unroll
            for (int al = 0; al < K1; ++al) {
              b1[al] = D1[(size_t)al * N + i]; b2[al] = D2[(size_t)al * N + i];
              dx = fma(cxJ[al], b1[al], dx); dy = fma(cyJ[al], b1[al], dy);
              ddx = fma(cxJ[al], b2[al], ddx); ddy = fma(cyJ[al], b2[al], ddy);
            }
            const double s2 = dx * dx + dy * dy, inv3 = 1.0 / (s2 * sqrt(s2));
            const double kp = (dx * ddy - dy * ddx) * inv3;
#if RL_G2_WEIGHTED
            k2p = fma(kp * wi, kp, k2p);
#else
            k2p = fma(kp, kp, k2p);
#endif
            double Gr[K1], ga = 0.0;
#pragma unroll
            for (int al = 0; al < K1; ++al) {
              const double nx = nus[2 * J[al]], ny = nus[2 * J[al] + 1];
              Gr[al] = ((b1[al] * nx) * ddy + dx * (b2[al] * ny) - (b1[al] * ny) * ddx - dy * (b2[al] * nx)) * inv3 -
                       3.0 * kp * (dx * b1[al] * nx + dy * b1[al] * ny) / s2;
              ga = fma(Gr[al], avs[J[al]], ga);
            }
            const double res = kp - ga;
            int e = 0;
#pragma unroll
            for (int al = 0; al < K1; ++al) {
#if RL_G2_WEIGHTED
              const double gw = Gr[al] * wi;
#pragma unroll
              for (int be = 0; be <= al; ++be) { acc[e] = fma(gw, Gr[be], acc[e]); ++e; }
              acc[NE + al] = fma(gw, res, acc[NE + al]);
#else
#pragma unroll
              for (int be = 0; be <= al; ++be) { acc[e] = fma(Gr[al], Gr[be], acc[e]); ++e; }
              acc[NE + al] = fma(Gr[al], res, acc[NE + al]);
#endif
            }
          }
        }
        k2p = wave_sum(k2p);
        if (lane == 0) red[wave] = k2p;
#pragma unroll
        for (int r0 = 0; r0 < NE + K1; r0 += GR) {
          const int w = NE + K1 - r0 < GR ? NE + K1 - r0 : GR;
          if (has) {
#pragma unroll
            for (int o = 0; o < GR; ++o)
              if (r0 + o < NE + K1) Spart[tid * GR + o] = acc[r0 + o];
          }
          __syncthreads();
          if (r0 == 0) {
            k2_last = red_sum(0);
            if (outer == 0) k2_first = k2_last;
            if (outer == RL_G2_N_OUTER) break;
          }
          g2_reduce_round<GR>(tid, nt, np, sch, Spart, Ssum, NO, r0, w);
          __syncthreads();
        }
        if (outer == RL_G2_N_OUTER) break;
      }
      // [Oc]  the chunk's constraint rows are (re)loaded here, after the register-hungry curvature
      // pass, so that they are not live across it; the laundered pointer keeps the loads in the loop
      rows.load(a.A, row0, cnt);
      if (has) {
        double xJ[K1];
#pragma unroll
        for (int al = 0; al < K1; ++al) xJ[al] = avs[J[al]];
#pragma unroll
        for (int r = 0; r < R; ++r) { RL_ROW_FENCE();
          double Av[K1], ax = 0.0;
          rows.get(r, Av);
#pragma unroll
          for (int al = 0; al < K1; ++al) ax = fma(Av[al], xJ[al], ax);
          const double2 lh = r < cnt ? reinterpret_cast<const double2*>(lohi)[row0 + r] : make_double2(-1.0, 1.0);
          if (outer == 0) {
            sl[r] = fmax(ax - lh.x, 1e-2); su[r] = fmax(lh.y - ax, 1e-2);
            ll[r] = 1.0; lu[r] = 1.0;
          } else {  // warm start from the previous linearisation's slacks and duals
            sl[r] = fmax(sl[r], 1e-2); su[r] = fmax(su[r], 1e-2);
            ll[r] = fmax(ll[r], 1e-2); lu[r] = fmax(lu[r], 1e-2);
          }
        }
      }
      __syncthreads();
      const double *xc = xsA, *xn = xsB;  // x is double buffered: [I8] reads it while the LA wave writes the next one
      for (int it = 0; it < a.max_ipm; ++it) {
        G2_LAP(5);
        // [I1]  three sweeps over the rows, one per flush round: only GR accumulators are live at a time
        {
          double dmv[R], ev[R], dlv[R];
#pragma unroll
          for (int r0 = 0; r0 < NO; r0 += GR) {
            const int w = NO - r0 < GR ? NO - r0 : GR;
            double acc[GR];
#pragma unroll
            for (int o = 0; o < GR; ++o) acc[o] = 0.0;
            if (r0 == 0) {
              double mu = 0.0, rpmax = 0.0;
              if (has) {
                double xJ[K1];
#pragma unroll
                for (int al = 0; al < K1; ++al) xJ[al] = xc[J[al]];
#pragma unroll
                for (int r = 0; r < R; ++r) { RL_ROW_FENCE();
                  dmv[r] = 0.0; ev[r] = 0.0; dlv[r] = 0.0;
                  if (r < cnt) {
                    double Av[K1], ax = 0.0;
                    rows.get(r, Av);
#pragma unroll
                    for (int al = 0; al < K1; ++al) ax = fma(Av[al], xJ[al], ax);
                    const double2 lh = reinterpret_cast<const double2*>(lohi)[row0 + r];
                    const double rpl = ax - lh.x - sl[r], rpu = lh.y - ax - su[r];
                    const double ql = ll[r] * frcp(sl[r]), qu = lu[r] * frcp(su[r]);
                    dmv[r] = ql + qu; ev[r] = qu * rpu - ql * rpl; dlv[r] = lu[r] - ll[r];
                    mu += sl[r] * ll[r] + su[r] * lu[r];
                    rpmax = fmax(rpmax, fmax(fabs(rpl), fabs(rpu)));
                  }
                }
              }
              mu = wave_sum(mu); rpmax = wave_max(rpmax);
              if (lane == 0) { red[wave] = mu; red[32 + wave] = rpmax; }
            }
            if (has) {
#pragma unroll
              for (int r = 0; r < R; ++r) { RL_ROW_FENCE();
                // rows beyond cnt have A = 0 and dm = e = dl = 0: they add nothing
                double Av[K1];
                rows.get(r, Av);
                int o = 0;
#pragma unroll
                for (int al = 0; al < K1; ++al) {
                  const double wa = dmv[r] * Av[al];
#pragma unroll
                  for (int be = 0; be <= al; ++be) {
                    if (o >= r0 && o < r0 + GR) acc[o - r0] = fma(wa, Av[be], acc[o - r0]);
                    ++o;
                  }
                  if (NE + al >= r0 && NE + al < r0 + GR) acc[NE + al - r0] = fma(Av[al], ev[r], acc[NE + al - r0]);
                  if (NE + K1 + al >= r0 && NE + K1 + al < r0 + GR)
                    acc[NE + K1 + al - r0] = fma(Av[al], dlv[r], acc[NE + K1 + al - r0]);
                }
              }
#pragma unroll
              for (int o = 0; o < GR; ++o)
                if (r0 + o < NO) Spart[tid * GR + o] = acc[o];
            }
            __syncthreads();
            g2_reduce_round<GR>(tid, nt, np, sch, Spart, Ssum, NO, r0, w);
            __syncthreads();
          }
        }
        G2_LAP(0);
        // [I2]
        if constexpr (G == 1) {
          g2_assemble_band<K>(tid, nt, np, Pc, Ssum, rdP, band, rd, rhs);
          __syncthreads();
          TwoFront<BW>::fill_images(tid, nt, itab, band, Mf);
        } else g2_assemble<K, G>(tid, nt, np, Pc, Ssum, rdP, Mf, rd, rhs);
        __syncthreads();
        G2_LAP(2);   // assembly of the normal matrix (all threads) up to its barrier
        // [I3]
        __syncthreads();
        G2_LAP(1);
        if (ctl[0] != 0.0) break;
        ++total_it;
        // [I4]..[I8]  Nothing but the slacks and duals is carried across a barrier: every pass rebuilds
        // the row quantities it needs from x, the affine direction dxa and the final direction dxs.
        struct RowAff { double rpl, rpu, isl, isu, d_sl, d_su, d_ll, d_lu; };
        auto row_affine = [&](int r, const double (&Av)[K1], const double (&xJ)[K1], const double (&aJ)[K1]) {
          RowAff f;
          double ax = 0.0, adx = 0.0;
#pragma unroll
          for (int al = 0; al < K1; ++al) { ax = fma(Av[al], xJ[al], ax); adx = fma(Av[al], aJ[al], adx); }
          const double2 lh = reinterpret_cast<const double2*>(lohi)[row0 + r];
          f.rpl = ax - lh.x - sl[r]; f.rpu = lh.y - ax - su[r];
          f.isl = frcp(sl[r]); f.isu = frcp(su[r]);
          f.d_sl = adx + f.rpl; f.d_su = f.rpu - adx;
          f.d_ll = (-(sl[r] * ll[r]) - ll[r] * f.d_sl) * f.isl;
          f.d_lu = (-(su[r] * lu[r]) - lu[r] * f.d_su) * f.isu;
          return f;
        };
        // [I4]+[I5]  one pass: step-length / complementarity statistics of the affine direction AND the
        // corrector partials.  The corrector weight is affine in sigma*mu,
        //   w = w0 + smu (1/sl - 1/su),   w0 = (-(sl ll + dsl dll) - ll rpl)/sl - (-(su lu + dsu dlu) - lu rpu)/su,
        // so A'w0 and A'(1/sl - 1/su) are accumulated side by side (2 (K+1) outputs) and the LA wave, which
        // computes sigma from the statistics, combines them.
        {
          double c1 = 0.0, c2 = 0.0, rmax = 0.0;
          double acc[2 * K1];
#pragma unroll
          for (int o = 0; o < 2 * K1; ++o) acc[o] = 0.0;
          if (has) {
            double xJ[K1], aJ[K1];
#pragma unroll
            for (int al = 0; al < K1; ++al) { xJ[al] = xc[J[al]]; aJ[al] = dxa[J[al]]; }
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (r < cnt) {
                double Av[K1];
                rows.get(r, Av);
                const RowAff f = row_affine(r, Av, xJ, aJ);
                rmax = fmax(rmax, fmax(fmax(-f.d_sl * f.isl, -f.d_su * f.isu),
                                       fmax(-f.d_ll * __builtin_amdgcn_rcp(ll[r]), -f.d_lu * __builtin_amdgcn_rcp(lu[r]))));
                c1 += sl[r] * f.d_ll + ll[r] * f.d_sl + su[r] * f.d_lu + lu[r] * f.d_su;
                c2 += f.d_sl * f.d_ll + f.d_su * f.d_lu;
                const double w0 = (-(sl[r] * ll[r] + f.d_sl * f.d_ll) - ll[r] * f.rpl) * f.isl -
                                  (-(su[r] * lu[r] + f.d_su * f.d_lu) - lu[r] * f.rpu) * f.isu;
                const double w1 = f.isl - f.isu;
#pragma unroll
                for (int al = 0; al < K1; ++al) {
                  acc[al] = fma(Av[al], w0, acc[al]);
                  acc[K1 + al] = fma(Av[al], w1, acc[K1 + al]);
                }
              }
            }
#pragma unroll
            for (int o = 0; o < 2 * K1; ++o) Spart[tid * GR + o] = acc[o];
          }
          c1 = wave_sum(c1); c2 = wave_sum(c2); rmax = wave_max(rmax);
          if (lane == 0) { red[wave] = c1; red[16 + wave] = c2; red[32 + wave] = rmax; }
        }
        __syncthreads();
        g2_reduce_round<GR>(tid, nt, np, sch, Spart, Ssum, NO, NE, 2 * K1);
        __syncthreads();
        G2_LAP(3);
        // [I6]
        __syncthreads();
        G2_LAP(4);
        const double smu = ctl[1];
        // [I7], [I8]
        auto row_final = [&](int r, const double (&xJ)[K1], const double (&aJ)[K1], const double (&dJ)[K1],
                             double& d_sl, double& d_su, double& d_ll, double& d_lu, double& isl, double& isu) {
          double Av[K1];
          rows.get(r, Av);
          const RowAff f = row_affine(r, Av, xJ, aJ);
          double adx = 0.0;
#pragma unroll
          for (int al = 0; al < K1; ++al) adx = fma(Av[al], dJ[al], adx);
          const double rcl = sl[r] * ll[r] - smu + f.d_sl * f.d_ll, rcu = su[r] * lu[r] - smu + f.d_su * f.d_lu;
          d_sl = adx + f.rpl; d_su = f.rpu - adx;
          d_ll = (-rcl - ll[r] * d_sl) * f.isl; d_lu = (-rcu - lu[r] * d_su) * f.isu;
          isl = f.isl; isu = f.isu;
        };
        {
          double rmax = 0.0;
          if (has) {
            double xJ[K1], aJ[K1], dJ[K1];
#pragma unroll
            for (int al = 0; al < K1; ++al) { xJ[al] = xc[J[al]]; aJ[al] = dxa[J[al]]; dJ[al] = dxs[J[al]]; }
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (r < cnt) {
                double d_sl, d_su, d_ll, d_lu, isl, isu;
                row_final(r, xJ, aJ, dJ, d_sl, d_su, d_ll, d_lu, isl, isu);
                rmax = fmax(rmax, fmax(fmax(-d_sl * isl, -d_su * isu),
                                       fmax(-d_ll * __builtin_amdgcn_rcp(ll[r]), -d_lu * __builtin_amdgcn_rcp(lu[r]))));
              }
            }
          }
          rmax = wave_max(rmax);
          if (lane == 0) red[32 + wave] = rmax;
        }
        __syncthreads();
        {
          const double rmax = red_max(2);
          const double alpha = rmax > 0.995 ? 0.995 / rmax : 1.0;
          if (has) {
            double xJ[K1], aJ[K1], dJ[K1];
#pragma unroll
            for (int al = 0; al < K1; ++al) { xJ[al] = xc[J[al]]; aJ[al] = dxa[J[al]]; dJ[al] = dxs[J[al]]; }
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (r < cnt) {
                double d_sl, d_su, d_ll, d_lu, isl, isu;
                row_final(r, xJ, aJ, dJ, d_sl, d_su, d_ll, d_lu, isl, isu);
                sl[r] = fma(alpha, d_sl, sl[r]); su[r] = fma(alpha, d_su, su[r]);
                ll[r] = fma(alpha, d_ll, ll[r]); lu[r] = fma(alpha, d_lu, lu[r]);
              }
            }
          }
        }
        __syncthreads();
        { const double* t_ = xc; xc = xn; xn = t_; }
      }
      // [Od]
      __syncthreads();
    }
#ifdef RL_G2_PROFILE
    if (tid == 0) for (int i = 0; i < 6; ++i) ctl[1 + i] = (double)rT[i];
#endif
    // ---- outputs of the row waves: line samples and the largest bound violation
    {
      const double* __restrict__ D0 = a.trk.D;
      double viol = -INFINITY, nact = 0.0;
      if (has) {
        for (int r = 0; r < cnt; ++r) {
          const int i = row0 + r;
          double x = 0.0, y = 0.0;
#pragma unroll
          for (int al = 0; al < K1; ++al) {
            const double h = D0[(size_t)al * N + i];
            x = fma(cxs[sp0 + al], h, x); y = fma(cys[sp0 + al], h, y);
          }
          if (a.out_xy) reinterpret_cast<double2*>(a.out_xy)[(size_t)b * N + i] = make_double2(x, y);
          const double lat = (x - a.trk.base[i]) * a.trk.base[(size_t)2 * N + i] +
                             (y - a.trk.base[(size_t)N + i]) * a.trk.base[(size_t)3 * N + i];
          const double2 lh = reinterpret_cast<const double2*>(lohi)[i];
          viol = fmax(viol, fmax(lh.x - lat, lat - lh.y));
          if (lat - lh.x < 1e-6 || lh.y - lat < 1e-6) nact += 1.0;
        }
      }
      viol = wave_max(viol); nact = wave_sum(nact);
      if (lane == 0) { red[32 + wave] = viol; red[wave] = nact; }
    }
    __syncthreads();
  } else {
    // ========================================================================= linear-algebra wave
    FoldBand<BW, G> fb;   // np > 64 (G == 3): the folded band over G groups of 64 rows (unused, hence eliminated, for G == 1)
    TwoFront<BW> tf;      // np <= 64 (G == 1): two fronts in this one wave
    double last_step = 0.0;
#ifdef RL_G2_PROFILE
    long long tF = 0, tS = 0, tA = 0, tk = 0;
#define G2_TIC() tk = wall_clock64()
#define G2_TOC(acc) acc += wall_clock64() - tk
#else
#define G2_TIC()
#define G2_TOC(acc)
#endif
    for (int outer = 0;; ++outer) {
      // [Oa]
      for (int j = tid; j < n; j += nt) {
        const int jj = j >= np ? j - np : j;
        cxs[j] = fma(avs[jj], nus[2 * jj], a.trk.c0[jj]);
        cys[j] = fma(avs[jj], nus[2 * jj + 1], a.trk.c0[n + jj]);
      }
      __syncthreads();
      // [Ob]
      bool done = false;
#pragma unroll
      for (int r0 = 0; r0 < NE + K1; r0 += GR) {
        const int w = NE + K1 - r0 < GR ? NE + K1 - r0 : GR;
        __syncthreads();
        if (r0 == 0) {
          k2_last = red_sum(0);
          if (outer == 0) k2_first = k2_last;
          if (outer == RL_G2_N_OUTER) { done = true; break; }
        }
        g2_reduce_round<GR>(tid, nt, np, sch, Spart, Ssum, NO, r0, w);
        __syncthreads();
      }
      if (done) break;
      // [Oc]  P = sc 2 G'G + eps I (cyclic band: Pc[j][d] = P[j][j-d]),  q = sc 2 G'(kappa - G a)
      double qinf = 0.0;
      {
        double tr = 0.0;
        for (int task = lane; task < np * K1; task += kWave) {
          const int j = task / K1, d = task - j * K1;
          double sum = 0.0;
          for (int al = d; al <= K; ++al) {
            int sp = j - al;
            if (sp < 0) sp += np;
            sum += Ssum[sp * NO + al * (al + 1) / 2 + (al - d)];
          }
          Pc[task] = 2.0 * sum;
          if (d == 0) tr += 2.0 * sum;
        }
        tr = wave_sum(tr);
        const double sc = (double)np / tr;
        for (int task = lane; task < np * K1; task += kWave) {
          const int d = task % K1;
          Pc[task] = Pc[task] * sc + (d == 0 ? 1e-9 : 0.0);
        }
        for (int j = lane; j < np; j += kWave) {
          double sum = 0.0;
          for (int al = 0; al <= K; ++al) {
            int sp = j - al;
            if (sp < 0) sp += np;
            sum += Ssum[sp * NO + NE + al];
          }
          const double q = 2.0 * sum * sc;
          qv[j] = q;
          xsA[j] = avs[j];
          qinf = fmax(qinf, fabs(q));
        }
        qinf = wave_max(qinf);
      }
      __syncthreads();
      double *xc = xsA, *xn = xsB;
      for (int it = 0; it < a.max_ipm; ++it) {
        // [I1]  rdP = P x + q
        for (int j = lane; j < np; j += kWave) {
          double s = qv[j];
#pragma unroll
          for (int d = 0; d <= K; ++d) {
            int jm = j - d; if (jm < 0) jm += np;
            s = fma(Pc[j * K1 + d], xc[jm], s);
            if (d > 0) { int jp = j + d; if (jp >= np) jp -= np; s = fma(Pc[jp * K1 + d], xc[jp], s); }
          }
          rdP[j] = s;
        }
#pragma unroll
        for (int r0 = 0; r0 < NO; r0 += GR) {
          const int w = NO - r0 < GR ? NO - r0 : GR;
          __syncthreads();
          g2_reduce_round<GR>(tid, nt, np, sch, Spart, Ssum, NO, r0, w);
          __syncthreads();
        }
        // [I2]
        const double mu_sum = red_sum(0), rpmax = red_max(2);
        if constexpr (G == 1) {
          g2_assemble_band<K>(tid, nt, np, Pc, Ssum, rdP, band, rd, rhs);
          __syncthreads();
          TwoFront<BW>::fill_images(tid, nt, itab, band, Mf);
        } else g2_assemble<K, G>(tid, nt, np, Pc, Ssum, rdP, Mf, rd, rhs);
        __syncthreads();
        // [I3]
        bool conv;
        {
          double rdmax = 0.0;
          for (int j = lane; j < np; j += kWave) rdmax = fmax(rdmax, fabs(rd[j]));
          rdmax = wave_max(rdmax);
          const double mu = mu_sum / (double)(2 * N);
          // the exit rule (rl_device.hpp: ipm_done): the complementarity alone, 1e-7 before the last linearisation, 1e-10 on it
          (void)rdmax; (void)rpmax; (void)qinf;
          conv = ipm_done(kIpmTolOneOffset, outer + 1 >= RL_G2_N_OUTER && !a.last_as_mid, mu);
          if (lane == 0) ctl[0] = conv ? 1.0 : 0.0;
        }
        double bx[G];
        if (!conv) {
          if constexpr (G == 1) {
            G2_TIC();
            tf.load(Mf, lane);
            tf.factor(np, lane, Mf + (2 * BW + 1) * 64, rhs);   // + forward substitution of the affine right-hand side
            G2_TOC(tF);
            G2_TIC();
            double yt_, yb_, ym_;
            tf.first_y(yt_, yb_, ym_);
            tf.backward(np, lane, yt_, yb_, ym_, dxa);
            G2_TOC(tS);
          } else {
            G2_TIC();
            fb.load(Mf, lane);
            fb.factor(np, lane);
            G2_TOC(tF);
            G2_TIC();
#pragma unroll
            for (int q = 0; q < G; ++q) { const int p = lane + 64 * q; bx[q] = p < np ? rhs[fold_inv(p, np)] : 0.0; }
            fb.solve(np, lane, bx);
            G2_TOC(tS);
#pragma unroll
            for (int q = 0; q < G; ++q) { const int p = lane + 64 * q; if (p < np) dxa[fold_inv(p, np)] = bx[q]; }
          }
        }
        __syncthreads();
        if (conv) break;
        ++total_it;
        // [I4]+[I5]
        __syncthreads();
        g2_reduce_round<GR>(tid, nt, np, sch, Spart, Ssum, NO, NE, 2 * K1);
        __syncthreads();
        // [I6]  sigma from the affine statistics, second right-hand side, solve
        double smu;
        {
          const double c1 = red_sum(0), c2 = red_sum(1), rmax = red_max(2);
          const double aaff = rmax > 0.995 ? 0.995 / rmax : 1.0;
          const double mu = mu_sum / (double)(2 * N);
          const double mu_aff = (mu_sum + aaff * c1 + aaff * aaff * c2) / (double)(2 * N);
          const double ratio = mu_aff / mu;
          smu = ratio * ratio * ratio * mu;
          if (lane == 0) ctl[1] = smu;
        }
        if constexpr (G == 1) {
          // second right-hand side in the natural order of the unknowns, through LDS (rhs is free after the first solve)
          if (lane < np) {
            const int j = lane;
            double v = 0.0, v1 = 0.0;
            for (int al = 0; al <= K; ++al) {
              int sp = j - al;
              if (sp < 0) sp += np;
              v += Ssum[sp * NO + NE + al];
              v1 += Ssum[sp * NO + NE + K1 + al];
            }
            rhs[j] = fma(smu, v1, v) - rd[j];
          }
          wave_lds_fence();
          G2_TIC();
          double yt_, yb_, ym_;
          tf.forward(np, lane, rhs, yt_, yb_, ym_);
          tf.backward(np, lane, yt_, yb_, ym_, dxs);
          G2_TOC(tS);
        } else {
#pragma unroll
          for (int q = 0; q < G; ++q) {
            const int p = lane + 64 * q;
            double v = 0.0;
            if (p < np) {
              const int j = fold_inv(p, np);
              double v1 = 0.0;
              for (int al = 0; al <= K; ++al) {
                int sp = j - al;
                if (sp < 0) sp += np;
                v += Ssum[sp * NO + NE + al];
                v1 += Ssum[sp * NO + NE + K1 + al];
              }
              v = fma(smu, v1, v) - rd[j];
            }
            bx[q] = v;
          }
          G2_TIC();
          fb.solve(np, lane, bx);
          G2_TOC(tS);
#pragma unroll
          for (int q = 0; q < G; ++q) { const int p = lane + 64 * q; if (p < np) dxs[fold_inv(p, np)] = bx[q]; }
        }
        __syncthreads();
        // [I7]
        __syncthreads();
        // [I8]
        {
          const double rmax = red_max(2);
          const double alpha = rmax > 0.995 ? 0.995 / rmax : 1.0;
          for (int j = lane; j < np; j += kWave) xn[j] = fma(alpha, dxs[j], xc[j]);
        }
        __syncthreads();
        { double* t_ = xc; xc = xn; xn = t_; }
      }
      // [Od]
      {
        double stepmax = 0.0;
        for (int j = lane; j < np; j += kWave) { stepmax = fmax(stepmax, fabs(xc[j] - avs[j])); avs[j] = xc[j]; }
        last_step = wave_max(stepmax);
      }
      __syncthreads();
    }
    // ---- outputs of the linear-algebra wave: control points, offsets, statistics
    for (int j = lane; j < n; j += kWave)
      reinterpret_cast<double2*>(a.out_ctrl)[(size_t)b * n + j] = make_double2(cxs[j], cys[j]);
    if (a.out_a)
      for (int j = lane; j < np; j += kWave) a.out_a[(size_t)b * np + j] = avs[j];
    __syncthreads();
    if (lane == 0) {
      double* st = a.out_stats + (size_t)b * 8;
      st[0] = (double)total_it; st[1] = k2_first; st[2] = k2_last; st[3] = red_max(2); st[4] = last_step;
#if RL_G2_WEIGHTED
      st[5] = red_sum(0); st[6] = refused; st[7] = 0.0;
#else
      st[5] = red_sum(0); st[6] = 0.0; st[7] = 0.0;
#endif
#ifdef RL_G2_PROFILE
      st[5] = (double)tF; st[6] = (double)tS; st[7] = ctl[6]; st[1] = ctl[1]; st[2] = ctl[2]; st[3] = ctl[3]; st[4] = ctl[4] + 1e-3 * ctl[5];
#endif
    }
  }
}
#undef RL_G2_N_OUTER
