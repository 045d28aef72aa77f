// Body of conv_wgrad_wino_kernel / conv_wgrad_wino_grouped_kernel / conv_wgrad_wino_ap_kernel / conv_wgrad_wino_pair_kernel /
// conv_wgrad_wino_shared_kernel (textually included,
// see conv3x3_wgrad_halo_body.inc). Expects: template parameter TPR; `a` (WgWinoArgs); `nwg_` = workgroups of this problem and `bid_` = this
// workgroup's index among them (blockIdx.x except in the pair and shared kernels, whose later problems start behind the first); constexpr bool AP and
// `ap` (lvae_bn_apply): with AP the dY operand does not exist yet — it is dy = BN'(ap.dh; ap.x) * ap.drop, the BatchNorm-backward apply
// that would otherwise run as a launch of its own in front of this one (round 5): the kernel reduces the producer's partial rows, forms dy
// while it stages a chunk and (the input-channel block 0 workgroups) stores it to ap.out for the dgrad that follows. Cout == 64 only.
// a.ncib = blocks of 32 input channels of the problem (C1 / 32: 1 or 2; with AP always 2): the workgroup's block, the owner of the bias
// partial (block 0) and the slab index [range][ncib][ncog] come from it, and C1 = 32 * ncib is x's pixel stride.
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int W = 2 * TPR, HW2 = W + 2, TR = 16 / TPR, HROWS = 2 * TR + 2;
  constexpr int HP = HROWS * HW2;                      // halo pixels of a chunk
  constexpr int XSLOTS = (HP * 8 + 511) / 512;         // float4 slots per thread (32 channels per pixel)
  constexpr int BUF = HP * WG_XS + 64 * WG_DS;         // floats per LDS buffer
  const lvae_conv_desc& d = a.d;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5, pi = wave & 3, kg = wave >> 2;
  int bid = bid_;
  {
    const int nwg = nwg_, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int ncib = AP ? 2 : a.ncib, xcs = 32 * ncib;   // xcs: x's pixel stride (floats)
  const int cib = bid & (ncib - 1), cog = (bid >> (ncib - 1)) % a.ncog, range = (bid >> (ncib - 1)) / a.ncog;
  const int c_begin = range * a.cpr;
  const int c_end = min(a.total_chunks, c_begin + a.cpr);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#ifdef LVAE_WGW_DBG  // compile-time phase-skip mask of the profiling builds (tools/wgrad_ab.sh); never defined in the product
  constexpr int dbg = LVAE_WGW_DBG;  // 1: no global loads, 2: no MFMAs, 4: no slab stores, 8: no input transform, 16: no epilogue at all
#else
  constexpr int dbg = 0;
#endif

  // ---- staging plan: x halo slots (pixel, float4 of this block's 32 channels), two dy slots (pixel, float4 of 64 channels)
  const int xc4 = (t & 7) * 4;
  // (AP: recomputed where used instead of held in 4 x XSLOTS registers — that variant has none to spare; HW2 is a compile-time constant)
  int xrel[AP ? 1 : XSLOTS], xhy[AP ? 1 : XSLOTS];
  bool xcol_ok[AP ? 1 : XSLOTS], xin[AP ? 1 : XSLOTS];
  auto slot = [&](int u, int& hy, bool& col_ok, bool& in, int& rel) {
    const int px = (t >> 3) + 64 * u;
    hy = px / HW2;
    const int hx = px - hy * HW2;
    in = px < HP;
    col_ok = (hx >= 1) & (hx <= W);
    rel = (hy * W + hx) * xcs + cib * 32 + xc4;  // relative to the pixel (row oh0 - 1, column -1) of the image
  };
  if (!AP) {
#pragma unroll
    for (int u = 0; u < XSLOTS; ++u) slot(u, xhy[u], xcol_ok[u], xin[u], xrel[u]);
  }
  const int dpx = t >> 4, dc4 = (t & 15) * 4;     // second slot: pixel + 32
  const int drel = dpx * d.Cout + cog * 64 + dc4;  // dy chunk rows are contiguous in memory (full image width)
  const bool dy_ok = cog * 64 + dc4 < d.Cout;
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = zero4;
  if (d.in_scale && !AP) {   // (AP: the two vectors are read from LDS where they are used — that variant has no register to spare)
    sc = *reinterpret_cast<const f32x4*>(d.in_scale + cib * 32 + xc4);
    sh = *reinterpret_cast<const f32x4*>(d.in_shift + cib * 32 + xc4);
  }
  f32x4 xreg[XSLOTS], dreg[2];
  f32x4 yreg[AP ? 2 : 1], dmask = {1.f, 1.f, 1.f, 1.f};
  float* Cf = smem + 2 * BUF;   // (AP) the apply's coefficient rows (bn_apply.h), then in_scale and in_shift [2][64], behind the two chunk buffers,
                                // inside the allocation the epilogue's exchange sizes (131 KB); in registers they spilled a kernel that sits at 234-242 of 256
  if (AP) {
    // This kernel's own copy of ap_reduce (bn_apply.h) with its in_scale / in_shift rows in front of the first barrier, kept word for word:
    // through the shared helper the 32-pixel-wide instantiations, which sit at 256 registers, spill 5 values instead of 4 and take 5 % longer.
    const int q = t & 31, rg = t >> 5, rows = ap.rows;
    f32x4 accp = zero4;
    for (int r = rg; r < rows; r += 16 * 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int rr = r + 16 * u;
        v[u] = *reinterpret_cast<const f32x4*>(ap.parts + (size_t)(rr < rows ? rr : 0) * 128 + q * 4);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r + 16 * u < rows) accp += v[u];
    }
    *reinterpret_cast<f32x4*>(smem + rg * 128 + q * 4) = accp;   // [16][128], in front of the (still unused) chunk buffers
    if (t < 256) Cf[t] = ap.coef[t];
    if (t < 64) {
      Cf[AP_CF + t] = d.in_scale ? d.in_scale[t] : 1.f;
      Cf[AP_CF + 64 + t] = d.in_scale ? d.in_shift[t] : 0.f;
    }
    __syncthreads();
    if (t < 64) {
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int g2 = 0; g2 < 16; ++g2) {
        sa += (double)smem[g2 * 128 + t];
        sb += (double)smem[g2 * 128 + 64 + t];
      }
      const BnBwdChannel r = bn_bwd_finish(sa, sb, ap.M);
      Cf[AP_C1 + t] = r.c1;
      Cf[AP_C2 + t] = r.c2;
      if (bid_ == 0) {
        if (ap.dbeta) ap.dbeta[t] += r.dbeta;
        if (ap.dgamma) ap.dgamma[t] += r.dgamma;
      }
    }
    __syncthreads();   // the scratch is read and Cf is published: the first chunk may be staged
  }
  const float* dysrc = AP ? ap.dh : a.dy;
  unsigned xok = 0;
  auto load_chunk = [&](int c) {
    const int n = fastdiv(c, a.m_cpi), cr = c - n * a.cpi;
    const int oh0 = cr * (2 * TR);
    const float* xb = d.x + ((int64_t)(n * d.H + oh0 - 1) * W - 1) * xcs;
    xok = 0;
#pragma unroll
    for (int u = 0; u < XSLOTS; ++u) {
      int s_hy, s_rel;
      bool s_col, s_in;
      if (AP) slot(u, s_hy, s_col, s_in, s_rel);
      else { s_hy = xhy[u]; s_col = xcol_ok[u]; s_in = xin[u]; s_rel = xrel[u]; }
      const int ih = oh0 - 1 + s_hy;
      const bool ok = s_in & s_col & ((unsigned)ih < (unsigned)d.H);
      const float* p = ok ? xb + s_rel : d.x;
      if (dbg & 1) xreg[u] = zero4;
      else xreg[u] = *reinterpret_cast<const f32x4*>(p);
      xok |= ok ? (1u << u) : 0u;
    }
    const int64_t doff0 = (int64_t)(n * d.H + oh0) * W * d.Cout + drel;
    const float* dyb = dy_ok ? dysrc + doff0 : dysrc;  // channels >= Cout read as zero
    if (dbg & 1) {
      dreg[0] = dreg[1] = zero4;
    } else {
      dreg[0] = *reinterpret_cast<const f32x4*>(dyb);
      dreg[1] = *reinterpret_cast<const f32x4*>(dy_ok ? dyb + 32 * d.Cout : dyb);
    }
    if (AP) {
      const float* yb = dy_ok ? ap.x + doff0 : ap.x;
      yreg[0] = *reinterpret_cast<const f32x4*>(yb);
      yreg[AP ? 1 : 0] = *reinterpret_cast<const f32x4*>(dy_ok ? yb + 32 * d.Cout : yb);
      if (ap.drop) dmask = *reinterpret_cast<const f32x4*>(ap.drop + (size_t)n * d.Cout + (dy_ok ? cog * 64 + dc4 : 0));
    }
    if (!dy_ok) dreg[0] = dreg[1] = zero4;
  };
  auto store_chunk = [&](float* buf, int c) {
    if (AP) {
      const int n = fastdiv(c, a.m_cpi), cr = c - n * a.cpi;
      const int64_t doff0 = (int64_t)(n * d.H + cr * (2 * TR)) * W * d.Cout + drel;
      const ApRows cf = ap_rows(Cf, dc4);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        f32x4 v = ap_value4(cf, dreg[k], yreg[AP ? k : 0], ap.act) * dmask;
        if (!dy_ok) v = zero4;
        dreg[k] = v;
        if (cib == 0 && dy_ok) store_wt4(ap.out + doff0 + (k ? 32 * d.Cout : 0), v);
      }
    }
    if (AP) {
      sc = *reinterpret_cast<const f32x4*>(Cf + AP_CF + cib * 32 + xc4);
      sh = *reinterpret_cast<const f32x4*>(Cf + AP_CF + 64 + cib * 32 + xc4);
    }
#pragma unroll
    for (int u = 0; u < XSLOTS; ++u) {
      if (AP ? ((t >> 3) + 64 * u < HP) : xin[u]) {
        f32x4 v = zero4;
        if ((xok >> u) & 1u) {
          v = xreg[u];
          if (d.in_scale && !(dbg & 8)) v = act_fwd4(v * sc + sh, d.in_act);
        }
        *reinterpret_cast<f32x4*>(buf + ((t >> 3) + 64 * u) * WG_XS + xc4) = v;
      }
    }
    *reinterpret_cast<f32x4*>(buf + HP * WG_XS + dpx * WG_DS + dc4) = dreg[0];
    *reinterpret_cast<f32x4*>(buf + HP * WG_XS + (dpx + 32) * WG_DS + dc4) = dreg[1];
  };

  // ---- per-lane read bases: tile = 8*kg + 2*ss + lh of the chunk
  // B^T rows: [1,0,-1,0], [0,1,1,0], [0,-1,1,0], [0,1,0,-1]  ->  t = d[ra] + sgn * d[rb]
  const int ra = pi == 0 ? 0 : (pi == 2 ? 2 : 1);
  const int rb = pi == 0 ? 2 : (pi == 1 ? 2 : (pi == 2 ? 1 : 3));
  const float sgn = pi == 1 ? 1.f : -1.f;
  // row i of A (4x2) = [[1,0],[1,1],[1,-1],[0,-1]]  ->  s = alpha * dy[0] + beta * dy[1]
  const float alpha = pi == 3 ? 0.f : 1.f;
  const float beta = pi == 0 ? 0.f : (pi == 1 ? 1.f : -1.f);
  int xbase_px, dbase_px;
  if (TPR == 4) {
    xbase_px = 4 * kg * HW2 + 2 * lh;
    dbase_px = 4 * kg * W + 2 * lh;
  } else if (TPR == 8) {
    xbase_px = 2 * kg * HW2 + 2 * lh;
    dbase_px = 2 * kg * W + 2 * lh;
  } else {
    xbase_px = 16 * kg + 2 * lh;
    dbase_px = 16 * kg + 2 * lh;
  }
  const int xoff_a = (xbase_px + ra * HW2) * WG_XS + li;
  const int xoff_b = (xbase_px + rb * HW2) * WG_XS + li;
  const int doff = HP * WG_XS + dbase_px * WG_DS + li;

  f32x16 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][h][r] = 0.f;
  float dbacc[2] = {0.f, 0.f};

  if (c_begin < c_end) {
    load_chunk(c_begin);
    store_chunk(smem, c_begin);
    if (c_begin + 1 < c_end) load_chunk(c_begin + 1);
  }
  __syncthreads();
  for (int c = c_begin; c < c_end; ++c) {
    const float* buf = smem + ((c - c_begin) & 1) * BUF;
    const float* pa = buf + xoff_a;
    const float* pb = buf + xoff_b;
    const float* pd = buf + doff;
    // LDS reads of k-step ss+1 are issued before the MFMAs of k-step ss (their latency hides under 512 MFMA cycles)
    float rxa[4], rxb[4], ry[2][4];
    auto read_step = [&](int ss) {
      const int cx = TPR == 4 ? 2 * (ss >> 1) * HW2 + 4 * (ss & 1) : 4 * ss;  // pixels
      const int cd = TPR == 4 ? 2 * (ss >> 1) * W + 4 * (ss & 1) : 4 * ss;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        rxa[cc] = pa[(cx + cc) * WG_XS];
        rxb[cc] = pb[(cx + cc) * WG_XS];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float* q = pd + cd * WG_DS + 32 * h;
        ry[h][0] = q[0];
        ry[h][1] = q[WG_DS];
        ry[h][2] = q[W * WG_DS];
        ry[h][3] = q[(W + 1) * WG_DS];
      }
    };
    read_step(0);
#pragma unroll
    for (int ss = 0; ss < 4; ++ss) {
      float tt[4], vv[4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) tt[cc] = __builtin_fmaf(sgn, rxb[cc], rxa[cc]);
      vv[0] = tt[0] - tt[2];
      vv[1] = tt[1] + tt[2];
      vv[2] = tt[2] - tt[1];
      vv[3] = tt[1] - tt[3];
      float ww[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float s0 = __builtin_fmaf(beta, ry[h][2], alpha * ry[h][0]), s1 = __builtin_fmaf(beta, ry[h][3], alpha * ry[h][1]);
        ww[h][0] = s0;
        ww[h][1] = s0 + s1;
        ww[h][2] = s0 - s1;
        ww[h][3] = -s1;
        dbacc[h] += ww[h][1];  // position (1,1) of A dY A^T is the plain sum of the 2x2 block (used from the pi == 1 waves)
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ss + 1 < 4) read_step(ss + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (dbg & 2) acc[j][h][0] += vv[j] * ww[h][j];
          else acc[j][h] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[j], ww[h][j], acc[j][h], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (c + 1 < c_end) {
      store_chunk(smem + ((c + 1 - c_begin) & 1) * BUF, c + 1);
      if (c + 2 < c_end) load_chunk(c + 2);
    }
    __syncthreads();
  }

  // ---- add the two tile halves through LDS (kg == 1 publishes, kg == 0 sums) and write the slab
  float* Rs = smem;  // [pi][j][h][r][64 lanes]
  if (dbg & 16) {
    float v = dbacc[0] + dbacc[1];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) v += acc[j][h][r];
    if (v == 12345.678f) a.slab_w[t] = v;
    return;
  }
  // Each wave of a tile-half pair (pi, kg) FINISHES one channel half (h = kg) and hands the other to its partner: half the LDS volume of
  // a one-sided exchange, and all eight waves store slab rows instead of four.
  auto hand_over = [&](auto hsel) {
    constexpr int h = decltype(hsel)::value;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) Rs[(((pi * 4 + j) * 2 + h) * 16 + r) * 64 + lane] = acc[j][h][r];
  };
  if (kg == 0) hand_over(std::integral_constant<int, 1>{});
  else hand_over(std::integral_constant<int, 0>{});
  if (kg == 1 && pi == 1) {
    Rs[4 * 4 * 2 * 16 * 64 + lane] = dbacc[0];
    Rs[4 * 4 * 2 * 16 * 64 + 64 + lane] = dbacc[1];
  }
  __syncthreads();
  // The wave holds a whole position row i = pi: the column half of G^T dU G is applied HERE, before the slab is written (linear, so it
  // commutes with the sum over slabs): 3 rows per (ci, i) instead of 4 = 25 % less slab traffic for the kernel and for the reduce;
  // row 4 i + 3 of the slab stays unwritten and unread. The reduce applies the row half.  G^T = [[1,.5,.5,0],[0,.5,-.5,0],[0,.5,.5,1]]
  float* slab = a.slab_w + (size_t)((range * ncib + cib) * a.ncog + cog) * 32 * 16 * 64 + 4 * pi * 64;
  auto finish = [&](auto hsel) {
    constexpr int h = decltype(hsel)::value;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = (r & 3) + 8 * (r >> 2) + 4 * lh;
      float u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = acc[j][h][r] + Rs[(((pi * 4 + j) * 2 + h) * 16 + r) * 64 + lane];
      const float g[3] = {u[0] + 0.5f * (u[1] + u[2]), 0.5f * (u[1] - u[2]), 0.5f * (u[1] + u[2]) + u[3]};
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (!(dbg & 4) || g[b] == 12345.678f) slab[((size_t)ci * 16 + b) * 64 + 32 * h + li] = g[b];
    }
  };
  if (kg == 0) finish(std::integral_constant<int, 0>{});
  else finish(std::integral_constant<int, 1>{});
  if (kg == 0) {
    if (pi == 1 && cib == 0 && a.slab_b) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float v = dbacc[h] + Rs[4 * 4 * 2 * 16 * 64 + 64 * h + lane];
        v += __shfl_xor(v, 32, 64);
        if (lh == 0) a.slab_b[(size_t)(range * a.ncog + cog) * 64 + 32 * h + li] = v;
      }
    }
  }
