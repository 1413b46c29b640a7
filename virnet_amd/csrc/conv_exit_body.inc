// conv_exit_body.inc -- the body of conv_exit_kernel / conv_exit_zadd_kernel (conv_exit.hip), included into both: `a` (FArgs), NCH,
// ZADD (constexpr bool) and `zadd` (the additive partial map, NULL without ZADD) are the including kernel's.  One text, two kernels: the
// plain kernels' code is what it was before the additive map existed (same instructions, tools/knobs.md VIRNET_TAIL_COMPOSE).
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nch = NCH ? NCH : (a.Cin >> 4);
  char* const a_lds = smem;                                      // [chunk][hi|lo][64 lanes][16 B]
  float* const z_lds = reinterpret_cast<float*>(smem + nch * 2048);   // [cout * 9 rows + 1 dummy][EX_ZS]

  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int tile = xcd * a.tiles_per_xcd + q;
  if (q >= a.tiles_per_xcd || tile >= a.ntiles) return;
  const int img = fast_div(tile, a.mg_tpi);
  const int trem = tile - img * (a.ntx * a.nty);
  const int ty = fast_div(trem, a.mg_ntx), tx = trem - ty * a.ntx;
  const int oy0 = ty * EX_TH, ox0 = tx * EX_TW;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int nrows = a.cout * 9;
  TSTAMP(0);

  if constexpr (NCH != 0) {                                       // (all pieces requested before the first lands: one round trip)
    f32x4 wv[NCH / 2];
#pragma unroll
    for (int i = 0; i < NCH / 2; ++i) wv[i] = *reinterpret_cast<const f32x4*>(a.wimg + i * 4096 + tid * 16);
#pragma unroll
    for (int i = 0; i < NCH / 2; ++i) *reinterpret_cast<f32x4*>(a_lds + i * 4096 + tid * 16) = wv[i];
  } else {
    for (int i = tid * 16; i < nch * 2048; i += 256 * 16) *reinterpret_cast<f32x4*>(a_lds + i) = *reinterpret_cast<const f32x4*>(a.wimg + i);
  }
  __syncthreads();
  TSTAMP(1);

  // thread = output pixel of the epilogue.  The residual's values (cout <= 3) are requested HERE, before the pixel blocks: they have landed
  // long before the shift-add wants them (requested there, they were one more HBM round trip between the barrier and the stores).
  const int oyl = tid >> 5, oxl = tid & 31;
  const int oy = oy0 + oyl, ox = ox0 + oxl;
  const bool inside = oy < a.crop_h && ox < a.crop_w;
  const size_t plane = (size_t)a.crop_h * a.crop_w;
  const size_t o0 = (size_t)img * a.cout * plane + (size_t)oy * a.crop_w + ox;
  // ... and the rows' inverse scales and the biases are read NOW, as scalars: behind the first store the compiler can no longer prove them
  // unchanged and reads them per channel with vector loads whose wait also waits for the previous channel's store (one more round trip each)
  float scv[27], bsv[3];
#pragma unroll
  for (int i = 0; i < 27; ++i) scv[i] = a.inv_scale[i];          // (the packed image always holds 32 scales)
#pragma unroll
  for (int c = 0; c < 3; ++c) bsv[c] = (a.bias && c < a.cout) ? a.bias[c] : 0.f;
  // ZADD: this lane's sixteen rows' scales 2^e = 1 / inv_scale (exact: the exponent field mirrored), requested with the scalars above
  [[maybe_unused]] float zsc[16];
  if constexpr (ZADD) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(a.inv_scale + 8 * j + 4 * lhi);
#pragma unroll
      for (int i = 0; i < 4; ++i) zsc[4 * j + i] = __builtin_bit_cast(float, 0x7f000000 - __builtin_bit_cast(int, s4[i]));
    }
  }
  float rv[3] = {0.f, 0.f, 0.f};
  if (a.nchw_op == VIRNET_NCHW_ADD && inside) {
    const int rw = a.crop_w / a.res_sf;
    const size_t rplane = (size_t)(a.crop_h / a.res_sf) * rw;
    const size_t r0 = (size_t)img * a.cout * rplane + (size_t)(oy / a.res_sf) * rw + ox / a.res_sf;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < a.cout) rv[c] = a.res[a.res_sf > 1 ? r0 + c * rplane : o0 + c * plane];
  }

  const float* const ximg = a.x + (size_t)img * a.H * a.W * a.Cin;
  float amax = 0.f;
  // block -> this lane's pixel pointer (NULL: outside the halo / the image: zeros)
  auto pixel_of = [&](int blk) -> const float* {
    const int p = blk * 32 + l31;
    const int hy = p / EX_HW, hx = p - hy * EX_HW;
    const int gy = oy0 - 1 + hy, gx = ox0 - 1 + hx;
    const bool valid = blk < EX_BLK && p < EX_HPX && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
    return valid ? ximg + ((size_t)gy * a.W + gx) * a.Cin + lhi * 8 : nullptr;
  };
  auto mma = [&](f32x16& acc, int c, f32x4 v0, f32x4 v1) {
    if (a.in_act) { v0 = lrelu4(v0, a.in_slope); v1 = lrelu4(v1, a.in_slope); }
    range_note(amax, v0, v1);
    h8 bh, bl;
    split8(v0, v1, bh, bl);
    const h8 ah = *reinterpret_cast<const h8*>(a_lds + c * 2048 + lane * 16);
    const h8 al = *reinterpret_cast<const h8*>(a_lds + c * 2048 + 1024 + lane * 16);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  };
  auto put_z = [&](int blk, const f32x16& acc) {
    // z[row][p] = the RAW accumulator (the row's inverse weight scale, a power of two, is applied by the shift-add: there it is a scalar
    // operand).  Accumulator register r of lane (l31, lhi) is row 8*(r>>2) + 4*lhi + (r&3), column l31; rows beyond the cout * 9 real ones
    // land in ONE dummy row behind them -- sixteen unconditional ds_write_b32.  (Round 5: the scale used to be read from global memory
    // here, one load + s_waitcnt vmcnt(0) per register inside the block loop -- sixteen dependent round trips per block, each of which
    // also drained the NEXT block's prefetched pixels: 42 of a workgroup's 55 k cycles, tools/exit_timeline.py.)
    const int p = blk * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * lhi + (r & 3);
      z_lds[min(row, nrows) * EX_ZS + p] = acc[r];
    }
  };
  if constexpr (NCH != 0) {
    // A wave owns blocks wave, wave + 4, wave + 8 (the last one: waves 0..2).  TWO blocks' pixels are in flight per wave (2 x NCH x 32 B per
    // lane, ping-pong register sets, no copies); buffer loads, so that a lane outside the halo / the image reads zeros through an
    // out-of-range offset -- no branch around the loads, and no wait for a load in flight before a masked lane's zero is written.
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg), 0, a.H * a.W * a.Cin * 4, 0x00020000);
    auto pixel_off = [&](int blk) -> unsigned {
      const int p = blk * 32 + l31;
      const int hy = p / EX_HW, hx = p - hy * EX_HW;
      const int gy = oy0 - 1 + hy, gx = ox0 - 1 + hx;
      const bool valid = p < EX_HPX && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
      return valid ? (unsigned)(((gy * a.W + gx) * a.Cin + lhi * 8) * 4) : 0x80000000u;
    };
    auto request = [&](unsigned off, f32x4 (&v0)[NCH], f32x4 (&v1)[NCH]) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        v0[c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off + c * 64, 0, 0));
        v1[c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, off + c * 64 + 16, 0, 0));
      }
    };
    auto compute = [&](int blk, f32x4 (&v0)[NCH], f32x4 (&v1)[NCH]) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) mma(acc, c, v0[c], v1[c]);
      put_z(blk, acc);
    };
    static_assert(EX_BLK > 8 && EX_BLK <= 12, "three blocks per wave at most, two at least");
    f32x4 p0[NCH], p1[NCH], q0[NCH], q1[NCH];
    const bool third = wave + 8 < EX_BLK;                 // (wave-uniform)
    if constexpr (!ZADD) {
      request(pixel_off(wave), p0, p1);
      request(pixel_off(wave + 4), q0, q1);
      compute(wave, p0, p1);
      if (third) request(pixel_off(wave + 8), p0, p1);
      compute(wave + 4, q0, q1);
      if (third) compute(wave + 8, p0, p1);
    } else {
      // the same walk; a block's request also asks for the lane's sixteen rows of zadd at its pixel (4 x 16 B: channels 8j + 4 lhi ..+3 =
      // accumulator registers 4j ..+3), and its accumulators start from them
      const auto zrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(zadd + (size_t)img * a.H * a.W * 32), 0, a.H * a.W * 128, 0x00020000);
      auto zadd_off = [&](int blk) -> unsigned {
        const int p = blk * 32 + l31;
        const int hy = p / EX_HW, hx = p - hy * EX_HW;
        const int gy = oy0 - 1 + hy, gx = ox0 - 1 + hx;
        const bool valid = p < EX_HPX && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        return valid ? (unsigned)(((gy * a.W + gx) * 32 + lhi * 4) * 4) : 0x80000000u;
      };
      auto request_z = [&](unsigned off, f32x4 (&z)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(zrs, off + j * 32, 0, 0));
      };
      auto compute_z = [&](int blk, f32x4 (&v0)[NCH], f32x4 (&v1)[NCH], const f32x4 (&z)[4]) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = z[r >> 2][r & 3] * zsc[r];
#pragma unroll
        for (int c = 0; c < NCH; ++c) mma(acc, c, v0[c], v1[c]);
        put_z(blk, acc);
      };
      f32x4 zp[4], zq[4];
      request(pixel_off(wave), p0, p1);
      request_z(zadd_off(wave), zp);
      request(pixel_off(wave + 4), q0, q1);
      request_z(zadd_off(wave + 4), zq);
      compute_z(wave, p0, p1, zp);
      if (third) { request(pixel_off(wave + 8), p0, p1); request_z(zadd_off(wave + 8), zp); }
      compute_z(wave + 4, q0, q1, zq);
      if (third) compute_z(wave + 8, p0, p1, zp);
    }
  } else {
    for (int blk = wave; blk < EX_BLK; blk += 4) {
      const float* const px = pixel_of(blk);
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      // (runtime chunk count: left rolled -- "#pragma unroll 2" here could not be honoured and warned in every build)
      for (int c = 0; c < nch; ++c) {
        f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (px) {
          v0 = *reinterpret_cast<const f32x4*>(px + c * 16);
          v1 = *reinterpret_cast<const f32x4*>(px + c * 16 + 4);
        }
        mma(acc, c, v0, v1);
      }
      put_z(blk, acc);
    }
  }
  TSTAMP(2);
  range_report(a.range_flag, amax);
  __syncthreads();
  TSTAMP(3);
#ifdef VIRNET_F16_TIMING
  if (a.tlog && tid == 0) {
    a.tlog[(size_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);     // HW_REG_HW_ID
    a.tlog[(size_t)blockIdx.x * 8 + 6] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);    // HW_REG_XCC_ID
  }
#endif

  // ---- shift-add + planar epilogue: thread = output pixel
  if (!inside) return;
  float outv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = bsv[c];
    const float* const zc = z_lds + (c < a.cout ? c * 9 : 0) * EX_ZS + oyl * EX_HW + oxl;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) v += zc[(dy * 3 + dx) * EX_ZS + dy * EX_HW + dx] * scv[c * 9 + dy * 3 + dx];
    if (a.nchw_op == VIRNET_NCHW_ADD) v += rv[c];
    else if (a.nchw_op == VIRNET_NCHW_EXPCLAMP) v = expf(fminf(fmaxf(v, a.clamp_lo), a.clamp_hi));
    outv[c] = v;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (c < a.cout) a.y_raw[o0 + c * plane] = outv[c];
#ifdef VIRNET_F16_TIMING
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  TSTAMP(4);
