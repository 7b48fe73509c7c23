// rl_global_kernel.hpp -- the body of k_global_qp, included TWICE by rl_global.hpp (no include guard): with RL_GQ_WEIGHTED 0 it
// is k_global_qp, token for token the kernel it always was (so are its registers and spills), with RL_GQ_WEIGHTED 1 it is
// k_global_qp_weighted.  Everything the two share is written once, here.

// ------------------------------------------------------------------------------------------------
// RL_GQ_WEIGHTED (k_global_qp_weighted): the cost is sum_i w[b][i] kappa_i^2, weights [B][N].  The weight enters the curvature
// pass alone, as (G w) G, (G w) res and (kappa w) kappa (rl_global2_kernel.hpp states why in that form).  The kernel validates
// its own weights with one block reduction in front of the first linearisation (every thread takes part: there are no roles
// here); a refused instance runs as n_outer = 0 (stats[1], stats[2] unspecified) and reports the number of refused weights in
// stats[6].
#if RL_GQ_WEIGHTED
#define RL_GQ_N_OUTER n_outer
template <int K, int MAXB>
__global__ void __launch_bounds__(MAXB) k_global_qp_weighted(GlobalArgs a, const double* __restrict__ weights) {
#else
#define RL_GQ_N_OUTER a.n_outer
template <int K, int MAXB>
__global__ void __launch_bounds__(MAXB) k_global_qp(GlobalArgs a) {
#endif
  constexpr int K1 = K + 1, NE = K1 * (K1 + 1) / 2, NO = NE + 2 * K1, R = kGRows;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int nt = blockDim.x, nw = nt >> 6;
  const int b = blockIdx.x;
  const int N = a.trk.N, n = a.trk.n, np = a.np, m = np - K;
  const GlobalLayout L = global_layout(K, n, np, nt);
  double *xs = lds + L.xs, *dxs = lds + L.dxs, *avs = lds + L.avs, *qv = lds + L.qv, *rdP = lds + L.rdP;
  double *rd = lds + L.rd, *rhs = lds + L.rhs, *dinv = lds + L.dinv, *cxs = lds + L.cxs, *cys = lds + L.cys;
  double *nus = lds + L.nus, *Pc = lds + L.Pc, *Lb = lds + L.Lb, *W = lds + L.W, *Ssum = lds + L.Ssum;
  double *Spart = lds + L.Spart, *red = lds + L.red;
  int* sch = reinterpret_cast<int*>(lds + L.sch);

  // block reductions: up to three values at once, two barriers
  auto reduce3 = [&](double& vsum, double& vmax, double& vmin) {
    vsum = wave_sum(vsum); vmax = wave_max(vmax); vmin = wave_min(vmin);
    if (lane == 0) { red[wave] = vsum; red[16 + wave] = vmax; red[32 + wave] = vmin; }
    __syncthreads();
    double s = 0.0, mx = -INFINITY, mn = INFINITY;
    for (int w = 0; w < nw; ++w) { s += red[w]; mx = fmax(mx, red[16 + w]); mn = fmin(mn, red[32 + w]); }
    __syncthreads();
    vsum = s; vmax = mx; vmin = mn;
  };
  auto span_of = [&](int j, int al) { const int sp = j - al; return sp < 0 ? sp + np : sp; };

  // this thread's chunk
  const bool has = tid < a.nc;
  int row0 = 0, cnt = 0, sp0 = 0;
  if (has) {
    const int2 c = reinterpret_cast<const int2*>(a.chunk)[tid];
    row0 = c.x & 0xffffff; cnt = (unsigned)c.x >> 24; sp0 = c.y;
  }
  int J[K1];
#pragma unroll
  for (int al = 0; al < K1; ++al) { J[al] = sp0 + al; if (J[al] >= np) J[al] -= np; }

  for (int j = tid; j < np; j += nt) { nus[2 * j] = a.nu[2 * j]; nus[2 * j + 1] = a.nu[2 * j + 1]; avs[j] = 0.0; }
  for (int j = tid; j <= np; j += nt) sch[j] = a.span_ch0[j];
  __syncthreads();

  const double* __restrict__ wid = a.widths + (size_t)b * N * 2;
  const double* __restrict__ D0 = a.trk.D;
  const double* __restrict__ D1 = a.trk.D + (size_t)K1 * N;
  const double* __restrict__ D2 = a.trk.D + (size_t)2 * K1 * N;
  double k2_first = 0.0, k2_last = 0.0, last_step = 0.0;
  int total_it = 0;

#if RL_GQ_WEIGHTED
  const double* __restrict__ wrow = weights + (size_t)b * N;
  double refused = 0.0;   // workgroup-uniform after the reduction
  {
    double z0 = 0.0, z1 = 0.0;
    for (int i = tid; i < N; i += nt) {
      const double w = wrow[i];
      if (!(w >= kWeightMin && w <= kWeightMax)) refused += 1.0;   // NaN fails both comparisons
    }
    reduce3(refused, z0, z1);
  }
  const int n_outer = __builtin_amdgcn_readfirstlane(refused != 0.0 ? 0 : a.n_outer);   // scalar, as a.n_outer is
#endif

  // interior-point state of this thread's rows
  double sl[R], su[R], ll[R], lu[R], rpl[R], rpu[R];

  for (int outer = 0;; ++outer) {
    // ---- current control points
    for (int j = tid; j < n; j += nt) {
      const int jj = j >= np ? j - np : j;
      cxs[j] = fma(avs[jj], nus[2 * jj], a.trk.c0[jj]);
      cys[j] = fma(avs[jj], nus[2 * jj + 1], a.trk.c0[n + jj]);
    }
    __syncthreads();
    // ---- curvature and its Gauss-Newton rows; G'G and G'(kappa - G a) per chunk
    double k2p = 0.0;
    {
      double acc[NE + K1];
#pragma unroll
      for (int o = 0; o < NE + K1; ++o) acc[o] = 0.0;
      if (has) {
        double cxJ[K1], cyJ[K1], nxJ[K1], nyJ[K1], avJ[K1];
#pragma unroll
        for (int al = 0; al < K1; ++al) {
          cxJ[al] = cxs[sp0 + al]; cyJ[al] = cys[sp0 + al];
          nxJ[al] = nus[2 * J[al]]; nyJ[al] = nus[2 * J[al] + 1]; avJ[al] = avs[J[al]];
        }
#pragma unroll 1
        for (int r = 0; r < cnt; ++r) {
          const int i = row0 + r;
#if RL_GQ_WEIGHTED
          const double wi = wrow[i];
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
#if RL_GQ_WEIGHTED
          k2p = fma(kp * wi, kp, k2p);
#else
          k2p = fma(kp, kp, k2p);
#endif
          double G[K1], ga = 0.0;
#pragma unroll
          for (int al = 0; al < K1; ++al) {
            const double nx = nxJ[al], ny = nyJ[al];
            G[al] = ((b1[al] * nx) * ddy + dx * (b2[al] * ny) - (b1[al] * ny) * ddx - dy * (b2[al] * nx)) * inv3 -
                    3.0 * kp * (dx * b1[al] * nx + dy * b1[al] * ny) / s2;
            ga = fma(G[al], avJ[al], ga);
          }
          const double res = kp - ga;
          int e = 0;
#pragma unroll
          for (int al = 0; al < K1; ++al) {
#if RL_GQ_WEIGHTED
            const double gw = G[al] * wi;
#pragma unroll
            for (int be = 0; be <= al; ++be) { acc[e] = fma(gw, G[be], acc[e]); ++e; }
            acc[NE + al] = fma(gw, res, acc[NE + al]);
#else
#pragma unroll
            for (int be = 0; be <= al; ++be) { acc[e] = fma(G[al], G[be], acc[e]); ++e; }
            acc[NE + al] = fma(G[al], res, acc[NE + al]);
#endif
          }
        }
      }
      double vmx = 0.0, vmn = 0.0;
      reduce3(k2p, vmx, vmn);
      if (outer == 0) k2_first = k2p;
      k2_last = k2p;
      if (outer == RL_GQ_N_OUTER) break;
      flush_outputs<NE + K1>(acc, has, tid, nt, np, sch, Spart, Ssum, NO, 0);
    }
    // ---- P = sc 2 G'G + eps I (cyclic band: Pc[j][d] = P[j][j-d]),  q = sc 2 G'(kappa - G a)
    for (int task = tid; task < np * K1; task += nt) {
      const int j = task / K1, d = task - j * K1;
      double sum = 0.0;
      for (int al = d; al <= K; ++al) sum += Ssum[span_of(j, al) * NO + al * (al + 1) / 2 + (al - d)];
      Pc[task] = 2.0 * sum;
    }
    for (int j = tid; j < np; j += nt) {
      double sum = 0.0;
      for (int al = 0; al <= K; ++al) sum += Ssum[span_of(j, al) * NO + NE + al];
      qv[j] = 2.0 * sum;
      xs[j] = avs[j];
    }
    __syncthreads();
    double tr = 0.0, qinf = 0.0, dummy = 0.0;
    for (int j = tid; j < np; j += nt) tr += Pc[j * K1];
    reduce3(tr, qinf, dummy);
    const double sc = (double)np / tr;
    qinf = 0.0;
    for (int task = tid; task < np * K1; task += nt) {
      const int d = task % K1;
      Pc[task] = Pc[task] * sc + (d == 0 ? 1e-9 : 0.0);
    }
    for (int j = tid; j < np; j += nt) { qv[j] *= sc; qinf = fmax(qinf, fabs(qv[j])); }
    tr = 0.0;
    reduce3(tr, qinf, dummy);
    // ---- interior point from x = a
    if (has) {
      double xJ[K1];
#pragma unroll
      for (int al = 0; al < K1; ++al) xJ[al] = xs[J[al]];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r < cnt) {
          const int i = row0 + r;
          const double* __restrict__ Ar = a.A + (size_t)i * K1;
          double ax = 0.0;
#pragma unroll
          for (int al = 0; al < K1; ++al) ax = fma(Ar[al], xJ[al], ax);
          const double2 w = reinterpret_cast<const double2*>(wid)[i];
          const double lo = -(w.y - a.margin), hi = w.x - a.margin;
          if (outer == 0) {
            sl[r] = fmax(ax - lo, 1e-2); su[r] = fmax(hi - ax, 1e-2);
            ll[r] = 1.0; lu[r] = 1.0;
          } else {  // warm start from the previous linearisation's slacks and duals
            sl[r] = fmax(sl[r], 1e-2); su[r] = fmax(su[r], 1e-2);
            ll[r] = fmax(ll[r], 1e-2); lu[r] = fmax(lu[r], 1e-2);
          }
          rpl[r] = ax - lo - sl[r]; rpu[r] = hi - ax - su[r];
        }
      }
    }
    for (int it = 0; it < a.max_ipm; ++it) {
      // ---- residuals, complementarity, and the span sums of A'DA, A'e, A'(lu - ll)
      for (int j = tid; j < np; j += nt) {
        double s = qv[j];
#pragma unroll
        for (int d = 0; d <= K; ++d) {
          int jm = j - d; if (jm < 0) jm += np;
          s = fma(Pc[j * K1 + d], xs[jm], s);
          if (d > 0) { int jp = j + d; if (jp >= np) jp -= np; s = fma(Pc[jp * K1 + d], xs[jp], s); }
        }
        rdP[j] = s;
      }
      for (int q = tid; q < K * np; q += nt) W[q] = 0.0;
      double mu = 0.0, rpmax = 0.0, amin = 1.0;
      {
        double acc[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[o] = 0.0;
        if (has) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if (r < cnt) {
              const double* __restrict__ Ar = a.A + (size_t)(row0 + r) * K1;
              double Av[K1];
#pragma unroll
              for (int al = 0; al < K1; ++al) Av[al] = Ar[al];
              const double ql = ll[r] / sl[r], qu = lu[r] / su[r];
              const double dm = ql + qu, e = qu * rpu[r] - ql * rpl[r], dl = lu[r] - ll[r];
              mu += sl[r] * ll[r] + su[r] * lu[r];
              rpmax = fmax(rpmax, fmax(fabs(rpl[r]), fabs(rpu[r])));
              int o = 0;
#pragma unroll
              for (int al = 0; al < K1; ++al) {
                const double wa = dm * Av[al];
#pragma unroll
                for (int be = 0; be <= al; ++be) { acc[o] = fma(wa, Av[be], acc[o]); ++o; }
                acc[NE + al] = fma(Av[al], e, acc[NE + al]);
                acc[NE + K1 + al] = fma(Av[al], dl, acc[NE + K1 + al]);
              }
            }
          }
        }
        reduce3(mu, rpmax, amin);
        flush_outputs<NO>(acc, has, tid, nt, np, sch, Spart, Ssum, NO, 0);
      }
      const double mu_sum = mu;
      mu /= (double)(2 * N);
      // ---- dual residual, first right-hand side, normal matrix into the band + border storage
      double rdmax = 0.0;
      for (int j = tid; j < np; j += nt) {
        double s1 = 0.0, s2 = 0.0;
        for (int al = 0; al <= K; ++al) {
          const int base = span_of(j, al) * NO + NE + al;
          s1 += Ssum[base]; s2 += Ssum[base + K1];
        }
        const double r = rdP[j] + s2;
        rd[j] = r;
        rhs[j] = s1 - rdP[j];
        rdmax = fmax(rdmax, fabs(r));
      }
      for (int task = tid; task < np * K1; task += nt) {
        const int j = task / K1, d = task - j * K1;
        double sum = Pc[task];
        for (int al = d; al <= K; ++al) sum += Ssum[span_of(j, al) * NO + al * (al + 1) / 2 + (al - d)];
        int r = j, c = j - d;
        if (c < 0) { r = c + np; c = j; }
        if (r < m) Lb[r * K1 + (r - c)] = sum; else W[(r - m) * np + c] = sum;
      }
      double d0 = 0.0, d1 = 0.0;
      reduce3(d0, rdmax, d1);
      (void)rdmax; (void)rpmax; (void)qinf;   // the residuals no longer decide anything (rl_device.hpp: ipm_done)
      if (ipm_done(kIpmTolOneOffset, outer + 1 >= RL_GQ_N_OUTER && !a.last_as_mid, mu)) break;
      ++total_it;
      // ---- factor, affine direction
      if (wave == 0) {
        band_factor<K>(Lb, W, dinv, np, lane);
        band_solve<K>(Lb, W, dinv, np, lane, rhs, dxs);
      }
      __syncthreads();
      double pl[R], pu[R];
      double c1 = 0.0, c2 = 0.0;
      amin = 1.0;
      if (has) {
        double dJ[K1];
#pragma unroll
        for (int al = 0; al < K1; ++al) dJ[al] = dxs[J[al]];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r < cnt) {
            const double* __restrict__ Ar = a.A + (size_t)(row0 + r) * K1;
            double adx = 0.0;
#pragma unroll
            for (int al = 0; al < K1; ++al) adx = fma(Ar[al], dJ[al], adx);
            const double d_sl = adx + rpl[r], d_su = rpu[r] - adx;
            const double d_ll = (-(sl[r] * ll[r]) - ll[r] * d_sl) / sl[r];
            const double d_lu = (-(su[r] * lu[r]) - lu[r] * d_su) / su[r];
            if (d_sl < 0.0) amin = fmin(amin, 0.995 * (-sl[r] / d_sl));
            if (d_su < 0.0) amin = fmin(amin, 0.995 * (-su[r] / d_su));
            if (d_ll < 0.0) amin = fmin(amin, 0.995 * (-ll[r] / d_ll));
            if (d_lu < 0.0) amin = fmin(amin, 0.995 * (-lu[r] / d_lu));
            pl[r] = d_sl * d_ll; pu[r] = d_su * d_lu;
            c1 += sl[r] * d_ll + ll[r] * d_sl + su[r] * d_lu + lu[r] * d_su;
            c2 += pl[r] + pu[r];
          }
        }
      }
      // mu_aff = sum (s + alpha ds)(l + alpha dl) / 2N, expanded in alpha so that one reduction does
      double c2s = c2, dmx = 0.0;
      reduce3(c1, dmx, amin);
      {
        double z0 = 0.0, z1 = 0.0;
        reduce3(c2s, z0, z1);
      }
      const double mu_aff = (mu_sum + amin * c1 + amin * amin * c2s) / (double)(2 * N);
      const double ratio = mu_aff / mu, sigma = ratio * ratio * ratio;
      const double smu = sigma * mu;
      // ---- corrector right-hand side
      {
        double acc[K1];
#pragma unroll
        for (int al = 0; al < K1; ++al) acc[al] = 0.0;
        if (has) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            if (r < cnt) {
              const double* __restrict__ Ar = a.A + (size_t)(row0 + r) * K1;
              const double rcl = sl[r] * ll[r] - smu + pl[r], rcu = su[r] * lu[r] - smu + pu[r];
              const double wv = (-rcl - ll[r] * rpl[r]) / sl[r] - (-rcu - lu[r] * rpu[r]) / su[r];
#pragma unroll
              for (int al = 0; al < K1; ++al) acc[al] = fma(Ar[al], wv, acc[al]);
            }
          }
        }
        flush_outputs<K1>(acc, has, tid, nt, np, sch, Spart, Ssum, NO, NE);
      }
      for (int j = tid; j < np; j += nt) {
        double s1 = 0.0;
        for (int al = 0; al <= K; ++al) s1 += Ssum[span_of(j, al) * NO + NE + al];
        rhs[j] = s1 - rd[j];
      }
      __syncthreads();
      if (wave == 0) band_solve<K>(Lb, W, dinv, np, lane, rhs, dxs);
      __syncthreads();
      // ---- step length and update
      double adxv[R], dllv[R], dluv[R];
      amin = 1.0;
      if (has) {
        double dJ[K1];
#pragma unroll
        for (int al = 0; al < K1; ++al) dJ[al] = dxs[J[al]];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r < cnt) {
            const double* __restrict__ Ar = a.A + (size_t)(row0 + r) * K1;
            double adx = 0.0;
#pragma unroll
            for (int al = 0; al < K1; ++al) adx = fma(Ar[al], dJ[al], adx);
            const double d_sl = adx + rpl[r], d_su = rpu[r] - adx;
            const double rcl = sl[r] * ll[r] - smu + pl[r], rcu = su[r] * lu[r] - smu + pu[r];
            const double d_ll = (-rcl - ll[r] * d_sl) / sl[r], d_lu = (-rcu - lu[r] * d_su) / su[r];
            if (d_sl < 0.0) amin = fmin(amin, 0.995 * (-sl[r] / d_sl));
            if (d_su < 0.0) amin = fmin(amin, 0.995 * (-su[r] / d_su));
            if (d_ll < 0.0) amin = fmin(amin, 0.995 * (-ll[r] / d_ll));
            if (d_lu < 0.0) amin = fmin(amin, 0.995 * (-lu[r] / d_lu));
            adxv[r] = adx; dllv[r] = d_ll; dluv[r] = d_lu;
          }
        }
      }
      {
        double z0 = 0.0, z1 = 0.0;
        reduce3(z0, z1, amin);
      }
      const double alpha = amin;
      if (has) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r < cnt) {
            sl[r] = fma(alpha, adxv[r] + rpl[r], sl[r]);
            su[r] = fma(alpha, rpu[r] - adxv[r], su[r]);
            ll[r] = fma(alpha, dllv[r], ll[r]);
            lu[r] = fma(alpha, dluv[r], lu[r]);
            rpl[r] *= 1.0 - alpha; rpu[r] *= 1.0 - alpha;
          }
        }
      }
      for (int j = tid; j < np; j += nt) xs[j] = fma(alpha, dxs[j], xs[j]);
      __syncthreads();
    }
    // ---- accept the QP solution as the next linearisation point
    double stepmax = 0.0, z0 = 0.0, z1 = 0.0;
    for (int j = tid; j < np; j += nt) stepmax = fmax(stepmax, fabs(xs[j] - avs[j]));
    reduce3(z0, stepmax, z1);
    last_step = stepmax;
    for (int j = tid; j < np; j += nt) avs[j] = xs[j];
    __syncthreads();
  }

  // ---- outputs: control points, line samples, offsets, statistics
  for (int j = tid; j < n; j += nt)
    reinterpret_cast<double2*>(a.out_ctrl)[(size_t)b * n + j] = make_double2(cxs[j], cys[j]);
  if (a.out_a)
    for (int j = tid; j < np; j += nt) a.out_a[(size_t)b * np + j] = avs[j];
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
      const double2 w = reinterpret_cast<const double2*>(wid)[i];
      viol = fmax(viol, fmax(-(w.y - a.margin) - lat, lat - (w.x - a.margin)));
      if (lat + (w.y - a.margin) < 1e-6 || (w.x - a.margin) - lat < 1e-6) nact += 1.0;
    }
  }
  double z1 = 0.0;
  reduce3(nact, viol, z1);
  if (tid == 0) {
    double* st = a.out_stats + (size_t)b * 8;
    st[0] = (double)total_it; st[1] = k2_first; st[2] = k2_last; st[3] = viol; st[4] = last_step;
#if RL_GQ_WEIGHTED
    st[5] = nact; st[6] = refused; st[7] = 0.0;
#else
    st[5] = nact; st[6] = 0.0; st[7] = 0.0;
#endif
  }
}
#undef RL_GQ_N_OUTER
