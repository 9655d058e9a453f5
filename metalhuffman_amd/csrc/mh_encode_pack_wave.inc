// mh_encode_pack_wave.inc -- the body of enc_pack_wave_kernel, included by mh_encode.hip once per
// kernel: with MH_PACK_IMAGES 0 it is the planar packer's text as it always stood (so that
// kernel compiles to what it did), with MH_PACK_IMAGES 1 the same packer over image planes:
// the workgroup mapping (img_unit), the source pointer, the descriptor and load_row's
// fetch (img_row<kPs>) differ, nothing behind the fetch does. In scope: px, nb, ncode,
// table, meta, tile_off, offsets, codes, codes_stride, ncode_wg, tile_tail and gray_stride
// (planar, with kVec and kPair) or im (images, with kPs; kVec = kPair = false).
  // ncode_wg: workgroups per frame (ncode rounded up to kPackWaves tiles): a workgroup's
  // waves pack tiles of ONE frame and share its table, at a fixed LDS address (the
  // gathers need no per-wave base: one VALU per symbol for the address)
  __shared__ uint32_t tab[256];
  __shared__ __attribute__((aligned(16))) uint32_t s_w[kPackWaves][kStepSlots];
  // the wave index as a provably uniform value (readfirstlane): the tile, its offsets and
  // the step cursor then live in SGPRs (SALU) instead of being carried per lane
  const uint32_t lane = threadIdx.x & 63u, k = lane >> 3, r = lane & 7u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#if MH_PACK_IMAGES
  uint32_t f, unit, img, plane;
  img_unit(im, blockIdx.x, ncode_wg, f, unit, img, plane);
  const uint32_t t = unit * kPackWaves + wave, ch = im.fc + plane, pitch = im.pitch;
  const uint32_t ps = kPs == kBytePs ? im.ps : kPs;
#else
  const uint32_t f = blockIdx.x / ncode_wg, t = (blockIdx.x - f * ncode_wg) * kPackWaves + wave;
#endif
  if (!(uint32_t)meta[(uint64_t)f * kMetaWords + 1]) return;  // rejected frame (workgroup-uniform): nothing written
  {
    // the frame's table as len << 16 | right-aligned code (the tree's words hold the
    // code left-aligned in 16 bits): two symbols' codes combine in one v_lshl_or
    const uint32_t e = table[(uint64_t)f * 256 + threadIdx.x];
    const uint32_t L = e & 0x1Fu;
    tab[threadIdx.x] = L ? (L << 16) | ((e >> 16) >> (16u - L)) : 0u;
  }
  lds_barrier();
  if (t >= ncode) return;  // wave-uniform padding past the frame's last tile; no barrier follows
  uint32_t *lw = s_w[wave];
  const uint32_t E = tile_off[(uint64_t)f * (ncode + 1) + t];
#if MH_PACK_IMAGES
  const uint8_t *gray = px.gray + img * im.image_stride;  // the image's first byte
#else
  const uint8_t *gray = px.gray + f * gray_stride;
#endif
  const uint64_t b0 = (uint64_t)t * kBatchTile;
  const uint32_t nsteps = (uint32_t)((min<uint64_t>(kBatchTile, nb - b0) + kStepBlocks - 1) / kStepBlocks);
  const uint32_t by0 = (uint32_t)(b0 / px.bw), bx0 = (uint32_t)(b0 - (uint64_t)by0 * px.bw);
  // one descriptor from the tile's first block row: 32-bit offsets for any frame
  const uint32_t yb = by0 * 8u;
#if MH_PACK_IMAGES
  // ... up to the image's last sample (tile_rows_img)
  const uint64_t span64 = (uint64_t)(px.H - yb - 1u) * pitch + (uint64_t)px.W * ps;
  const uint32_t span = (uint32_t)(span64 < kMaxTileSpan ? span64 : kMaxTileSpan);
  const __amdgpu_buffer_rsrc_t rg = enc_rsrc(gray + (uint64_t)yb * pitch, span);
#else
  const __amdgpu_buffer_rsrc_t rg = enc_rsrc(gray + (uint64_t)yb * px.W, (uint64_t)(px.H - yb) * px.W);
#endif
  // row r of block (bx + k, by) wrapped into the frame, zero when !live or past the frame
  // (32-bit block indices, nb < 2^26; the step's row offset uniform, r * W per lane
  // once, a wrapped block adds 8 W: no per-step v_mul_lo, which is quarter rate)
#if MH_PACK_IMAGES
  const uint32_t nb32 = (uint32_t)nb, w8 = 8u * pitch;
#else
  const uint32_t nb32 = (uint32_t)nb, w8 = 8u * px.W;
#endif
  const auto load_row = [&](uint32_t sbx, uint32_t sby, uint32_t sb, uint32_t kk, uint32_t rr, uint32_t rrW,
                            bool live) -> uint64_t {
    uint32_t bx = sbx + kk, dy = 0, doff = 0;
    if (px.bw >= kStepBlocks) {  // kk < kStepBlocks: one wrap at most
      const bool wrap = bx >= px.bw;
      bx = wrap ? bx - px.bw : bx;
      dy = wrap ? 8u : 0u;
      doff = wrap ? w8 : 0u;
    } else {
      const uint32_t d = bx / px.bw;
      bx -= d * px.bw;
      dy = d * 8u;
#if MH_PACK_IMAGES
      doff = dy * pitch;
#else
      doff = dy * px.W;
#endif
    }
    const uint32_t ys = sby * 8u - yb;  // uniform: the step's first block row in the descriptor
    const bool in = live && sb + kk < nb32 && ys + dy + rr < px.H - yb;
#if MH_PACK_IMAGES
    return img_row<kPs>(rg, ys * pitch + doff + rrW + bx * (8u * ps), in, min(8u, px.W - bx * 8u), span, ps, ch);
#else
    const uint32_t off = ys * px.W + doff + rrW + bx * 8u;
    if constexpr (kVec) {
      typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
      const v2u32 v = __builtin_amdgcn_raw_buffer_load_b64(rg, (int)(in ? off : kOob), 0, 0);
      return ((uint64_t)v.y << 32) | v.x;
    } else {
      uint64_t q = 0;
#pragma unroll
      for (uint32_t c = 0; c < 8; ++c)
        q |= (uint64_t)__builtin_amdgcn_raw_buffer_load_b8(rg, (int)(in && bx * 8u + c < px.W ? off + c : kOob), 0, 0)
             << (8 * c);
      return q;
    }
#endif
  };
  uint32_t first_unused;
  // the tile's first word starts with the previous block's last E % 32 bits: lanes 0-7
  // recompute that block's codes (the previous tile leaves the shared word to this one)
  // from its symbols, which the split kept for this (tile_tail: one 64-B read)
  uint32_t head = 0;
  const uint32_t r0 = E & 31u;
  if (r0) {  // wave-uniform; t > 0 here (tile 0 starts at bit 0)
    const __amdgpu_buffer_rsrc_t rt = enc_rsrc(tile_tail + ((uint64_t)f * ncode + t - 1u) * 8u, 64u);
    typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
    const v2u32 tv = __builtin_amdgcn_raw_buffer_load_b64(rt, (int)(lane < 8 ? lane * 8u : kOob), 0, 0);
    const uint64_t qp = ((uint64_t)tv.y << 32) | tv.x;
    uint32_t lenp = 0;
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t e = tab[(uint32_t)(qp >> (8 * j)) & 0xFFu];
      const uint32_t len = e >> 16;
      acc = (acc << len) | (e & 0xFFFFu);  // the lane's codes MSB-first, last 64 bits
      lenp += len;
    }
    if (lane >= 8) lenp = 0;
    // bits of lanes after this one in the block; the lane's last bit lands at word bit
    // 32 - r0 + after (bits before the word fall off the top)
    const uint32_t incp = wave_scan_dpp(lenp);
    const uint32_t after = __builtin_amdgcn_readlane(incp, 7) - incp;
    uint32_t h = lane < 8 && after < r0 ? (uint32_t)(acc << (32u - r0 + after)) : 0u;
    for (uint32_t o = 1; o < 8; o <<= 1) h |= __shfl_xor(h, o);
    head = __builtin_amdgcn_readfirstlane(h);
  }
  typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
  v4u32 *lq = reinterpret_cast<v4u32 *>(lw);
  // the step's words as quads: one 16-B LDS write / read and one 16-B store per lane
  const auto clear_words = [&](uint32_t first) {
    lq[lane] = v4u32{lane == 0 ? first : 0u, 0u, 0u, 0u};
    lq[64 + lane] = v4u32{0u, 0u, 0u, 0u};
    if (lane < kStepSlots / 4 - 128) lq[128 + lane] = v4u32{0u, 0u, 0u, 0u};
  };
  clear_words(bswap32(head));
  const __amdgpu_buffer_rsrc_t rw = enc_rsrc(codes + f * codes_stride, codes_stride);
  const __amdgpu_buffer_rsrc_t ro = enc_rsrc(offsets + (uint64_t)f * nb, nb * 4u);
  uint32_t pos = E;
  uint32_t sbx = bx0, sby = by0;
  uint32_t sb = (uint32_t)b0;
#if MH_PACK_IMAGES
  uint32_t rW = r * pitch;
#else
  uint32_t rW = r * px.W;
#endif
  asm volatile("" : "+v"(rW));  // kept as is (else folded back into (ys + r) * W per step)
  // row r of the pair (2 k, 2 k + 1) of the step starting at block (sbx, sby) = sb
  const auto load_pair = [&](uint32_t bx_, uint32_t by_, uint32_t sb_, bool live, uint64_t &qa, uint64_t &qb) {
    if constexpr (kPair) {
      uint32_t bx = bx_ + 2u * k, doff = 0, dy = 0;
      if (px.bw >= kStepBlocks) {
        const bool wrap = bx >= px.bw;
        bx = wrap ? bx - px.bw : bx;
        dy = wrap ? 8u : 0u;
        doff = wrap ? w8 : 0u;
      } else {
        const uint32_t d = bx / px.bw;
        bx -= d * px.bw;
        dy = d * 8u;
        doff = dy * px.W;
      }
      const uint32_t ys = by_ * 8u - yb;
      const bool in = live && sb_ + 2u * k < nb32 && ys + dy + r < px.H - yb;
      // both blocks are inside the frame when the first is (an even width, an even first block)
      const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(rg, (int)(in ? ys * px.W + doff + rW + bx * 8u : kOob), 0, 0);
      qa = ((uint64_t)v.y << 32) | v.x;
      qb = ((uint64_t)v.w << 32) | v.z;
    } else {
      qa = load_row(bx_, by_, sb_, 2u * k, r, rW, live);
      qb = load_row(bx_, by_, sb_, 2u * k + 1u, r, rW, live);
    }
  };
  uint64_t qa, qb;
  load_pair(sbx, sby, sb, true, qa, qb);
  for (uint32_t s = 0; s < nsteps; ++s) {
    // the next step's rows (a dead load past the tile's last step: fixed count)
    uint32_t nbx = sbx + kStepBlocks, nby = sby;
    while (nbx >= px.bw) {  // uniform; once per step at most when bw >= kStepBlocks
      nbx -= px.bw;
      ++nby;
    }
    uint64_t na, nbq;
    load_pair(nbx, nby, sb + kStepBlocks, s + 1 < nsteps, na, nbq);
    const uint32_t ba = sb + 2u * k;
    const bool on_a = ba < nb32, on_b = ba + 1u < nb32;
    // codes MSB-first: pairs of symbols in 32 bits (v_lshl_or), chunks of four in 64
    uint64_t ch[4];
    uint32_t cl[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint64_t v = row_symbols(h ? qb : qa, r, px.delta, px.init_byte, &first_unused);
      uint32_t pc[4], pl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t e0 = tab[(uint32_t)(v >> (16 * j)) & 0xFFu], e1 = tab[(uint32_t)(v >> (16 * j + 8)) & 0xFFu];
        const uint32_t l1 = e1 >> 16;
        pc[j] = ((e0 & 0xFFFFu) << l1) | (e1 & 0xFFFFu);
        pl[j] = (e0 >> 16) + l1;
      }
      ch[2 * h] = ((uint64_t)pc[0] << pl[1]) | pc[1];
      ch[2 * h + 1] = ((uint64_t)pc[2] << pl[3]) | pc[3];
      cl[2 * h] = pl[0] + pl[1];
      cl[2 * h + 1] = pl[2] + pl[3];
    }
    const uint32_t na_bits = on_a ? cl[0] + cl[1] : 0u, nb_bits = on_b ? cl[2] + cl[3] : 0u;
    // bit order: block 2 k (rows 0-7), then block 2 k + 1: one scan of A | B << 16 (each
    // half's sum over the wave <= 8,192), the pair's start and its A total by broadcast
    const uint32_t x = na_bits | (nb_bits << 16);
    const uint32_t S = wave_scan_dpp(x), ex = S - x;
    const uint32_t g = __shfl(ex, lane & ~7u), ge = __shfl(S, lane | 7u);
    const uint32_t Tw = __builtin_amdgcn_readlane(S, 63);
    const uint32_t T = (Tw & 0xFFFFu) + (Tw >> 16);
    const uint32_t start = (g & 0xFFFFu) + (g >> 16);             // the pair's first bit (step-relative)
    const uint32_t atot = (ge & 0xFFFFu) - (g & 0xFFFFu);         // block 2 k's bits
    const uint32_t pa = (g >> 16) + (ex & 0xFFFFu);                // this row of block 2 k
    const uint32_t pb = (g & 0xFFFFu) + atot + (ex >> 16);         // this row of block 2 k + 1
    // block offsets: lane r = 0 writes block 2 k's, lane r = 1 block 2 k + 1's
    const bool wo = r == 0 ? on_a : r == 1 ? on_b : false;
    __builtin_amdgcn_raw_buffer_store_b32(pos + start + (r == 1 ? atot : 0u), ro, (int)(wo ? (ba + r) * 4u : kOob), 0,
                                          0);
    const uint32_t rr = pos & 31u;
    if (!MH_DIAG_PACK_NO_OR && on_a) {
      or_bits(lw, rr + pa, ch[0], cl[0]);
      or_bits(lw, rr + pa + cl[0], ch[1], cl[1]);
    }
    if (!MH_DIAG_PACK_NO_OR && on_b) {
      or_bits(lw, rr + pb, ch[2], cl[2]);
      or_bits(lw, rr + pb + cl[2], ch[3], cl[3]);
    }
    wave_sync();
    // whole words out; the last partial word stays as the next step's first
    const uint32_t nfull = (rr + T) >> 5, w0 = pos >> 5, nq4 = nfull >> 2;
    const v4u32 q0 = lq[lane], q1 = lq[64 + lane];                    // words 4 lane .., 256 + 4 lane ..
    const uint32_t tail = lw[min(4u * nq4 + lane, kStepSlots - 1u)];  // lanes < nfull % 4: the last words
    const uint32_t carry = lw[nfull];
    __builtin_amdgcn_raw_buffer_store_b128(q0, rw, (int)(lane < nq4 ? (w0 + 4u * lane) * 4u : kOob), 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(q1, rw, (int)(64u + lane < nq4 ? (w0 + 256u + 4u * lane) * 4u : kOob), 0, 0);
    __builtin_amdgcn_raw_buffer_store_b32(tail, rw, (int)(lane < (nfull & 3u) ? (w0 + 4u * nq4 + lane) * 4u : kOob), 0,
                                          0);
    wave_sync();
    clear_words(carry);
    wave_sync();
    pos += T;
    qa = na;
    qb = nbq;
    sbx = nbx;
    sby = nby;
    sb += kStepBlocks;
  }
  // the last tile writes its partial last word, then the zero pad up to the byte count
  // rounded to words (the others leave that word to the next tile)
  if (t + 1 == ncode) {
    const uint32_t nw = (uint32_t)(((uint64_t)(pos + 7u) / 8u + MH_CODES_PAD + 3u) / 4u);
    const uint32_t w = (pos >> 5) + lane;
    const uint32_t val = lane == 0 ? lw[0] : 0u;
    __builtin_amdgcn_raw_buffer_store_b32(val, rw, (int)(w < nw ? w * 4u : kOob), 0, 0);
  }
