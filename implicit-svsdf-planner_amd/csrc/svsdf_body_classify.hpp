// svsdf_body_classify.hpp -- the body of k_classify and of the scaled k_classify_sc (svsdf_kernels.hpp); see
// svsdf_body_solve.hpp.  The including kernel defines SC and scl.
  extern __shared__ double classify_lds[];
  const TrajL tr = stage_traj(trg, classify_lds);
  const int start = ctl->start, count = ctl->count;
  const int lane = (int)(threadIdx.x & 63);
  // (wave-uniform trip count: the interior lanes of a wave take their indices together, below)
  for (int e0 = (int)((blockIdx.x * blockDim.x + threadIdx.x) & ~63u); e0 < count; e0 += gridDim.x * blockDim.x) {
    const int e = e0 + lane;
    const bool in_range = e < count;
    const int i = start + (in_range ? e : 0);
    const double px = px_[i], py = py_[i];
    const double sdf = sdf_[i], ts = t_[i];
    const bool inter = in_range && !(sdf > 0);
    double vx = 0.0, vy = 0.0, w = 0.0;
    if (in_range && sdf > 0) {  // outside case (SWM:921-924)
      int piece = 0;
      const Pose p = pose_at(tr, ts, piece);
      double rx, ry;
      if constexpr (SC) {
        double i00, i11;
        scale_inv(scl, ts, i00, i11);
        rel_scaled(p, px, py, i00, i11, rx, ry);
      } else {
        const double dx = px - p.x, dy = py - p.y;
        rx = p.cs * dx + p.sn * dy;
        ry = (-p.sn) * dx + p.cs * dy;
      }
      double gx, gy;
      shape_grad<SHAPE>(sp, rx, ry, gx, gy);
      res_sdf[i] = sdf; res_t[i] = ts; res_gx[i] = gx; res_gy[i] = gy;
    } else if (inter) {
      // interior: velocity at t* with the low-speed rescans (SWM:929-954)
      double sl;
      int piece = locate_local(tr, ts, 0, sl);
      piece_vel(tr.c + piece * 18, sl, vx, vy, w);
      if (sqrt(vx * vx + vy * vy + w * w) < 0.01) {
        if (ts < 0.1) {
          for (double t_scan = ts; t_scan <= tr.dur; t_scan += 0.1) {
            piece = locate_local(tr, t_scan, piece, sl);
            piece_vel(tr.c + piece * 18, sl, vx, vy, w);
            if (sqrt(vx * vx + vy * vy + w * w) >= 0.01) break;
          }
        } else if (ts > tr.dur - 0.1) {
          for (double t_scan = ts; t_scan >= 0; t_scan -= 0.1) {
            piece = locate_local(tr, t_scan, piece, sl);
            piece_vel(tr.c + piece * 18, sl, vx, vy, w);
            if (sqrt(vx * vx + vy * vy + w * w) >= 0.01) break;
          }
        }
      }
    }
    // compact interior indices, one block of consecutive ones per wave (one atomic for the wave instead of one per
    // point; neighbouring points keep neighbouring entries in the interior-sized arrays)
    const unsigned long long mi = __ballot(inter);
    if (mi == 0ull) continue;   // wave-uniform
    const int leader = __ffsll((long long)mi) - 1;
    int base_i = 0;
    if (lane == leader) base_i = atomicAdd(n_int, __popcll(mi));
    base_i = __shfl(base_i, leader, 64);
    const int ia_ = base_i + __popcll(mi & ((1ull << lane) - 1ull));
    const bool kept = inter && ia_ < icap;
    if (inter && !kept) {   // no room: dropped (reads as inactive); the host sees n_int > icap, grows the arrays and repeats
      res_sdf[i] = 1e300; res_t[i] = ts; res_gx[i] = 0.0; res_gy[i] = 0.0;
    }
    const unsigned long long mk = __ballot(kept);
    if (mk == 0ull) continue;
    const int leader2 = __ffsll((long long)mk) - 1;
    int base_a = 0;
    if (lane == leader2) base_a = atomicAdd(&ctl->n_active[0], __popcll(mk));
    base_a = __shfl(base_a, leader2, 64);
    if (kept) {
      const int a = base_a + __popcll(mk & ((1ull << lane) - 1ull));
      const size_t ia = (size_t)ia_;
      // SampleSet2D::initSet (SWM:73-103)
      double theta0 = atan2(vx, -vy);
      if (theta0 < 0) theta0 += 2 * kPI;
      gs.pt[ia] = i;
      gs.r[ia] = 10;               // r0 (SWM:927)
      gs.theta0[ia] = theta0;
      gs.theta_res[ia] = kPI + 0.1;
      gs.iter[ia] = 1;
      gs.nsamp[ia] = 0;
      gs.phase[ia] = kPhaseNew;
      gs.list[0][start + a] = ia_;
      res_t[i] = ts;  // real_t_star fallback
    }
  }
