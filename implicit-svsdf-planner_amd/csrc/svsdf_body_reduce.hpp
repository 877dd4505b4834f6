// svsdf_body_reduce.hpp -- the body of k_reduce and of the scaled k_reduce_sc (svsdf_kernels.hpp); see
// svsdf_body_solve.hpp.  The including kernel defines SC and scl.
  extern __shared__ double asm_lds[];
  __shared__ unsigned s_last;
  const bool one_block = gridDim.x == 1;   // up to 256 points (the reference's demo maps give 101 .. 139): nothing to wait for
  assemble_body<SC>(trg, px_, py_, P, res_sdf, res_t, res_gx, res_gy, safety_hor, weight_p, block_partials, nonfinite, asm_lds, fuse && one_block, scl);
  if (!fuse) return;
  const int N = trg->N;
  const int plen = 19 * N + 1;
  const int nblocks = (int)gridDim.x;
  double *sums = asm_lds + traj_lds_doubles(N);   // (the accumulator rows are free again: plen <= 4 plen doubles)
  if (!one_block) {
  __threadfence();   // this block's partials (and its non-finite count) are visible device-wide before its ticket is
  __syncthreads();
  if (threadIdx.x == 0) s_last = (atomicAdd(ticket, 1u) == gridDim.x - 1u) ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // (other blocks wrote the partials: read at device scope, past this CU's vector cache)
  auto part = [&](int e, int b) { return __hip_atomic_load(&block_partials[(size_t)e * nblocks + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  {
    // Up to 1024 points (the reference's own scale): one THREAD per entry.  k_final's wave leaves in lane 0, for lane
    // values p_b = 0.0 + partial[e][b] (b < nblocks <= 4, zero beyond), the tree ((p0 + p2) + (p1 + p3)) -- the xor steps
    // 32 .. 4 only add zeros to lanes 0 .. 3 -- so the same bits come from four independent loads per thread instead of a
    // dependent load + butterfly per entry, one entry after the other (that loop cost 60 us of a 480 us callback).
    for (int e = threadIdx.x; e < plen; e += blockDim.x) {
      double p[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) p[b] = (b < nblocks) ? 0.0 + part(e, b) : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[0] += 0.0; p[1] += 0.0; p[2] += 0.0; p[3] += 0.0; }   // xor 32, 16, 8, 4: the partners hold zeros
      sums[e] = (p[0] + p[2]) + (p[1] + p[3]);                                             // xor 2, then xor 1
    }
  }
  }  // !one_block (one block: assemble_body left sums[e] = 0.0 + its partial in place)
  __syncthreads();
  finish_body(sums, N, out, ctl, nbatch, it_end, nonfinite, reinterpret_cast<unsigned long long *>(out + out_partial));
  __threadfence();
  __syncthreads();
  if (host_out) copy_result_to_host(host_out, out, N, out_partial, out_doubles);
  if (threadIdx.x == 0 && !one_block) *ticket = 0u;
