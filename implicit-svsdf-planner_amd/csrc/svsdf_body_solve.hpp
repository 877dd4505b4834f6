// svsdf_body_solve.hpp -- the body of k_solve and of the scaled k_solve_sc (svsdf_kernels.hpp), included inside both kernels
// so that the rigid kernel is the very text it was before the scaled path existed (same instructions).  The including
// kernel defines SC (constexpr bool), scl (ScaleDev) and ltab_g (layer pose tables or null).  Not a header: no include guard, include nothing else.
  extern __shared__ double solve_lds[];
  int n;
  const long long total = qs_total(qs, n);
  if (total <= 0 || (long long)blockIdx.x * (((prune & 2) != 0) ? (blockDim.x >> 6) : (blockDim.x / G)) >= total) return;
  const int K = trg->K;
  const int nch = (K + kChunk - 1) / kChunk;
  stage_poly_edges<SHAPE>(sp, solve_lds);
  double *tab_lds = solve_lds + poly_lds_doubles<SHAPE>(sp.nverts);
  Pose *pose = reinterpret_cast<Pose *>(tab_lds);
  Chunk *chunks = reinterpret_cast<Chunk *>(tab_lds + 4 * (size_t)K);
  {
    const double *src = reinterpret_cast<const double *>(pose_g);
    for (int i = threadIdx.x; i < 4 * K; i += blockDim.x) tab_lds[i] = src[i];
    const double *srcc = reinterpret_cast<const double *>(chunks_g);
    for (int i = threadIdx.x; i < 4 * nch; i += blockDim.x) tab_lds[4 * (size_t)K + i] = srcc[i];
  }
  const TrajL tr = stage_traj(trg, tab_lds + 4 * (size_t)K + 4 * (size_t)nch);  // ends with __syncthreads
  // per-wave descent state behind the trajectory (16-byte aligned: the tables before it are whole doubles, rounded up)
  const size_t tables = poly_lds_doubles<SHAPE>(sp.nverts) + 4 * (size_t)K + 4 * (size_t)nch + (size_t)traj_lds_doubles(tr.N);
  char *wave_lds = reinterpret_cast<char *>(solve_lds + ((tables + 1) & ~(size_t)1)) + (threadIdx.x >> 6) * ladder_lds_bytes(G);
  const int li = Grp<G>::li();
  unsigned n_eval = 0, n_scan = 0, n_solved = 0, n_culled = 0, n_spec = 0;
  unsigned long long sc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // SVSDF_SITE_STATS builds only
#ifndef SVSDF_CLOCK_PROBE
#define SVSDF_CLOCK_PROBE 1
#endif
  const bool clk_probe = SVSDF_CLOCK_PROBE && work_idx == 0 && blockIdx.x == 0 && threadIdx.x < 64;   // (wave-uniform; BatchCtl::clk)
  // (the start values wait in the control block itself, not in four vector registers that would live through the whole kernel)
  volatile unsigned long long *clk = ctl->clk;
  if (clk_probe && threadIdx.x == 0) { clk[0] = (unsigned long long)clock64(); clk[1] = (unsigned long long)wall_clock64(); }
  // Work distribution: a wave's FIRST 64 / G queries are its own (wave index: no atomic), the following ones come from
  // the launch's cursor.  (All waves of a launch start together: with a fetch first, their 3000 atomics on one address
  // take ~ 12 ns each, one after the other -- the last wave would start ~ 37 us late, in every launch of the chain.)
  // `prune` bit 1 (round 6; launches of a few hundred queries, i.e. the main solve at the reference's own scale): ONE query per
  // wave -- the other lane groups stay empty -- so that every descent is "the wave's last open one" from its first pass on and
  // takes the fused pass (derivative + both signs of the ladder in one step: descend_from_seed) instead of two dependent
  // steps per pass.  The chip has a wave slot for every query there; the launch is a chain of dependent evaluations.
  const bool solo = (prune & 2) != 0;
  // `prune` bits 2 / 3: the launch carries the pose table of scan layer 2 / of layer 3 behind it (LayerTab, read by this wave only)
  if ((threadIdx.x & 63) == 0) {
    LayerTab *lt = wave_layer_tab<G>(wave_lds);
    lt->l2 = (prune & 4) ? ltab_g : nullptr;
    lt->l3 = (prune & 8) ? ltab_g + (size_t)K * kLayerSteps : nullptr;
  }
  prune &= 1;
  const long long per_wave = solo ? 1 : 64 / G;
  const long long n_static = (long long)gridDim.x * (blockDim.x >> 6) * per_wave;
  for (int guard = 0; guard < (1 << 26); ++guard) {
    long long wave_base, gq;
    if (guard == 0) {
      wave_base = (long long)((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * per_wave;
      gq = wave_base + (long long)((threadIdx.x & 63) / G);
    } else {
      gq = fetch_work<G>(&ctl->work[work_idx], wave_base, (int)per_wave) + n_static;
      wave_base += n_static;
    }
    if (wave_base >= total) break;
    double px = 0.0, py = 0.0;
    size_t slot = 0;
    bool live = gq < total && (long long)((threadIdx.x & 63) / G) < per_wave;
    if (live) live = qs_slot(qs, n, gq, slot);
    if (live) {
      px = qs.qx[slot]; py = qs.qy[slot];
      live = (px == px);  // NaN marks an unused slot (whole group)
    }
    // ---- choiceTInit layer 1 over the pose table (or the seed k_round already found for a GSIP sample)
    double best_d = 1e9;
    int best_k = 0x7fffffff;
    bool culled = false;
    const unsigned long long t_scan0 = SVSDF_SITE_CLOCK();
    if (live) {
    if (qs.seed_k) {
      best_k = qs.seed_k[slot];
      best_d = qs.seed_d[slot];
    }
    if (!qs.seed_k || best_k < 0) {   // no seed for this query (main points, cheap-bound samples, unscanned lazy samples)
      scan_layer1<SHAPE, G>(sp, pose, chunks, K, nch, px, py, prune, cull_thresh, best_d, best_k, culled, n_scan, nullptr, -1,
                            sc, rot, slack_max);
    }
    if (culled && li == 0) { out_sdf[slot] = best_d; out_t[slot] = 0.0; ++n_culled; }
    }  // live
    const bool on = live && !culled;
    SVSDF_SITE_CYCLES(sc, 8, t_scan0);
    double x = 0.0, fx = 0.0;
    descend_from_seed<SHAPE, G, U, SC>(tr, tk, sp, px, py, on, best_k, best_d, x, fx, n_eval, n_spec, sc, wave_lds, scl, true);   // whole wave
    if (on && li == 0) {
      out_sdf[slot] = fx;
      out_t[slot] = x;
      ++n_solved;
    }
  }
  if (clk_probe && threadIdx.x == 0) {
    clk[0] = (unsigned long long)clock64() - clk[0];
    clk[1] = (unsigned long long)wall_clock64() - clk[1];
  }
  unsigned long long te = (unsigned long long)n_eval + n_scan, ts = n_solved, tc = n_scan, tu = n_culled, tp = n_spec;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    te += __shfl_xor(te, m, 64); ts += __shfl_xor(ts, m, 64); tc += __shfl_xor(tc, m, 64); tu += __shfl_xor(tu, m, 64);
    tp += __shfl_xor(tp, m, 64);
  }
  if ((threadIdx.x & 63) == 0 && (te || tu)) {
    StatSlot *ss = stat_slot(ctl->stat);
    atomicAdd(&ss->evals, te); atomicAdd(&ss->solves, ts); atomicAdd(&ss->scan, tc);
    if (tu) atomicAdd(&ss->culled, tu);
    if (tp) atomicAdd(&ss->spec, tp);
  }
#ifdef SVSDF_SITE_STATS
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    unsigned long long v = sc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stat_slot(ctl->stat)->pad[i], v);
  }
#endif
