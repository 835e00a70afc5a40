// mlt_motion_kernels.inc -- prediction pictures on the device (include/mltcnn.h: mlt_picture_predict, mlt_picture_compensate): an integer-sample block motion search
// of the current picture in a reference picture, and quarter-sample motion compensation of the reference with a per-block field.  Included by mlt_kernels.hip.
//
// Everything is integer arithmetic with one defined rule (the header states it; fastintercu-vvc_amd/motion.py restates it in numpy), so the outputs are the same
// bytes on every device and in every reduction order.
//
// NO GLOBAL LOAD IS FORMED FROM AN UNCLAMPED COORDINATE.  Both kernels read the reference through R(x, y) = ref[clamp(y, 0, H - 1)][clamp(x, 0, W - 1)] while they
// STAGE a window into LDS (2-byte loads: a wrapped plane has any pitch and 2-byte alignment only); the loops behind the staging index LDS alone, inside the part of
// it that the staging wrote -- or, where stated, inside the kernel's LDS allocation with the value read discarded.  Blocks are clipped at the right and bottom
// border of the picture: a block is bw x bh samples, bw = min(B, W - x0), bh = min(B, H - y0).

// ---- motion_search_kernel: one workgroup (256 lanes) per block ----
// LDS (dynamic, sized by the host from (B, R): mlt_motion_search_lds): the window win[B + 2R][Wn] with Wn = B + 2R (even), sample (r, c) = R(x0 - R + c, y0 - R + r),
// rows [0, bh + 2R) staged; behind it the block cur[B][B], columns >= bw and rows >= bh zero; behind that the four waves' minima (32 bytes).  Window and block
// are stored with the sign bit flipped (v ^ 0x8000): the map from int16 to uint16 keeps every difference, so |a - b| of the int16 values "as they are" is the unsigned absolute difference v_sad_u16 adds up for two samples at once.
// Candidate c of the (2R + 1)^2 is (dy, dx) = (c / (2R + 1) - R, c % (2R + 1) - R); lane t takes c = t, t + 256, ...  Per candidate and block row the lane walks the
// row in PAIRS of samples: the block's pair is one dword of cur (the same address in every lane: a broadcast), the window's pair starts at element e = (y + dy + R) Wn
// + dx + R + 2p -- dword e >> 1, and for odd e the upper half of that dword and the lower half of the next, put together by v_alignbit_b32 (shift 0 or 16: no branch).
// Lanes of a wave hold consecutive dx, so two lanes share a dword and a 32-lane half reads 16 consecutive dwords: no bank conflict except where a wave's candidates
// wrap to the next dy.  The "next" dword of the last pair of a row lies at most two elements behind the row's last sample: in the next window row or, behind the last
// row, in cur -- inside the allocation; its upper half is shifted out (odd e) or the whole of it is not used (even e).  An odd bw ends in a half pair: both operands
// are masked to their lower sample.
// The lane's best candidate is the smallest 64-bit key  cost << 24 | (|dx| + |dy|) << 16 | (dy + 64) << 8 | (dx + 64)  -- the order (cost, |dx| + |dy|, dy, dx) of
// the rule as ONE unsigned compare, so the order of the reduction cannot matter: a wave reduction by shuffles, the four waves' minima through LDS, no atomics; lane 0
// writes the block's vector (one 4-byte store) and its cost (one 4-byte store).
__device__ __forceinline__ int motion_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void motion_search_kernel(const MotionSearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int B = 1 << a.block_l, R = a.range, Wn = B + 2 * R, nC = 2 * R + 1;
  uint16_t *win = (uint16_t *)smem;
  uint16_t *cur = win + (size_t)Wn * Wn;
  unsigned long long *wave_best = (unsigned long long *)(cur + B * B);   // [4]; 8-byte aligned: Wn^2 and B^2 are multiples of 4 elements
  const int x0 = (int)blockIdx.x << a.block_l, y0 = (int)blockIdx.y << a.block_l;
  const int bw = min(B, a.width - x0), bh = min(B, a.height - y0);
  const int tid = threadIdx.x;

  const int win_rows = bh + 2 * R;
  for (int i = tid; i < win_rows * Wn; i += 256) {
    const int r = i / Wn, c = i - r * Wn;
    const int gx = motion_clampi(x0 - R + c, 0, a.width - 1), gy = motion_clampi(y0 - R + r, 0, a.height - 1);
    win[i] = (uint16_t)a.ref[(size_t)gy * (size_t)a.ref_pitch + gx] ^ 0x8000u;
  }
  for (int i = tid; i < B * B; i += 256) {
    const int r = i >> a.block_l, c = i & (B - 1);
    uint16_t v = 0;
    if (r < bh && c < bw) v = (uint16_t)a.cur[(size_t)(y0 + r) * (size_t)a.cur_pitch + (x0 + c)] ^ 0x8000u;
    cur[i] = v;
  }
  __syncthreads();

  const uint32_t *win32 = (const uint32_t *)win, *cur32 = (const uint32_t *)cur;
  const int full = bw >> 1, half_b = B >> 1, half_w = Wn >> 1;
  unsigned long long best = ~0ull;
  for (int c = tid; c < nC * nC; c += 256) {
    const int dyi = c / nC, dxi = c - dyi * nC;
    const uint32_t sh = (uint32_t)(dxi & 1) << 4;   // Wn is even: the parity of a row's first element is dx's
    uint32_t sad = 0;
    for (int y = 0; y < bh; ++y) {
      const uint32_t *wd = win32 + (size_t)(y + dyi) * half_w + (dxi >> 1);
      const uint32_t *cd = cur32 + (size_t)y * half_b;
      uint32_t prev = wd[0];
      for (int p = 0; p < full; ++p) {
        const uint32_t next = wd[p + 1];
        sad = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbit(next, prev, sh), cd[p], sad);
        prev = next;
      }
      if (bw & 1) {   // the half pair: prev holds the sample in its lower (even e) or upper (odd e) half
        const uint32_t w = (prev >> sh) & 0xffffu;
        sad = __builtin_amdgcn_sad_u16(w, cd[full] & 0xffffu, sad);
      }
    }
    const int dx = dxi - R, dy = dyi - R;
    const uint32_t l1 = (uint32_t)(abs(dx) + abs(dy));
    const uint32_t cost = sad + (uint32_t)a.lambda * l1;   // <= 4096 x 65535 + 65535 x 128 < 2^32
    const unsigned long long key = ((unsigned long long)cost << 24) | ((unsigned long long)l1 << 16) | ((unsigned long long)(dy + 64) << 8) | (unsigned long long)(dx + 64);
    best = key < best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) wave_best[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) best = wave_best[w] < best ? wave_best[w] : best;
    const int dx = (int)(best & 0xff) - 64, dy = (int)((best >> 8) & 0xff) - 64;
    const size_t blk = (size_t)blockIdx.y * (size_t)a.bx + blockIdx.x;
    *(uint32_t *)(a.mv + 2 * blk) = (uint32_t)(uint16_t)(int16_t)(4 * dx) | ((uint32_t)(uint16_t)(int16_t)(4 * dy) << 16);   // {mvx, mvy}: the field is 4-byte aligned
    a.cost[blk] = (uint32_t)(best >> 24);
  }
}

// ---- picture_compensate_kernel: one workgroup (256 lanes) per tile of a block, a tile = at most 16 rows x 64 columns ----
// blockIdx.x = the block's column, blockIdx.y = block row x tiles-per-block + the tile inside the block (B = 64: four tiles of 16 rows; B = 32: two; else one).
// The tile's vector (mvx, mvy), ix = mvx >> 2, fx = mvx & 3 (likewise y).  LDS (static): the clamped window win[h + 7][w + 7], sample (r, c) =
// R(tx0 + ix - 3 + c, ty0 + iy - 3 + r); the horizontal pass t[r][x] = sum_k C[fx][k] win[r][x + k] as int32; the vertical pass v = sum_j C[fy][j] t[y + j][x],
// dst = clip(0, 1023, (v + 2048) >> 12).  |t| <= 112 x 32768, |v| <= 112 x 112 x 32768 < 2^31.
// Stores: a work item of the vertical pass is 8 consecutive samples of a tile row.  Tiles start at multiples of 8 samples, so on a plane whose base and pitch are
// multiples of 16 bytes (vec_dst: every plane mlt_picture_create makes) a WHOLE item is one aligned 16-byte store; an item the picture's right border cuts, and every
// item of another plane, is stored sample by sample.  No byte outside the width x height samples of dst is written.
// The reference is a.ref, or with a per-block table (a.ref_idx != NULL: mlt_picture_predict_refs, mlt_picture_compensate_refs) a.refs[a.ref_idx[block]] -- the
// host has checked every entry against the number of references.
__constant__ int8_t kMotionTaps[4][8] = {{0, 0, 0, 64, 0, 0, 0, 0}, {-1, 4, -10, 58, 17, -5, 1, 0}, {-1, 4, -11, 40, 40, -11, 4, -1}, {0, 1, -5, 17, 58, -10, 4, -1}};

#define MLT_MC_TILE_W 64
#define MLT_MC_TILE_H 16
#define MLT_MC_WIN_PITCH 72   // >= MLT_MC_TILE_W + 7

__global__ __launch_bounds__(256) void picture_compensate_kernel(const PictureCompensateArgs a) {
  __shared__ int16_t win[(MLT_MC_TILE_H + 7) * MLT_MC_WIN_PITCH];
  __shared__ __attribute__((aligned(16))) int32_t hor[(MLT_MC_TILE_H + 7) * MLT_MC_TILE_W];
  const int B = 1 << a.block_l;
  const int bi = blockIdx.x, bj = (int)blockIdx.y / a.tiles_y, tj = (int)blockIdx.y - bj * a.tiles_y;
  const int tx0 = bi << a.block_l, ty0 = (bj << a.block_l) + tj * MLT_MC_TILE_H;
  const int w = min(min(B, MLT_MC_TILE_W), a.width - tx0);
  const int h = min(min(B - tj * MLT_MC_TILE_H, MLT_MC_TILE_H), a.height - ty0);
  if (h <= 0 || w <= 0) return;   // a tile below the picture's bottom border (uniform over the workgroup: before any barrier)
  const int tid = threadIdx.x;
  const size_t blk = (size_t)bj * (size_t)a.bx + bi;
  const int mvx = a.mv[2 * blk], mvy = a.mv[2 * blk + 1];
  const int ix = mvx >> 2, fx = mvx & 3, iy = mvy >> 2, fy = mvy & 3;
  const int16_t *ref = a.ref;
  long ref_pitch = a.ref_pitch;
  if (a.ref_idx) {   // uniform over the workgroup
    const int r = a.ref_idx[blk];
    ref = r == 0 ? a.refs[0] : (r == 1 ? a.refs[1] : (r == 2 ? a.refs[2] : a.refs[3]));
    ref_pitch = r == 0 ? a.ref_pitches[0] : (r == 1 ? a.ref_pitches[1] : (r == 2 ? a.ref_pitches[2] : a.ref_pitches[3]));
  }

  const int ww = w + 7, wh = h + 7;
  for (int i = tid; i < ww * wh; i += 256) {
    const int r = i / ww, c = i - r * ww;
    const int gx = motion_clampi(tx0 + ix - 3 + c, 0, a.width - 1), gy = motion_clampi(ty0 + iy - 3 + r, 0, a.height - 1);
    win[r * MLT_MC_WIN_PITCH + c] = ref[(size_t)gy * (size_t)ref_pitch + gx];
  }
  __syncthreads();

  int cx[8], cy[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { cx[k] = kMotionTaps[fx][k]; cy[k] = kMotionTaps[fy][k]; }
  for (int i = tid; i < wh * MLT_MC_TILE_W; i += 256) {   // (columns >= w: zero -- a cut item's lanes beyond w read them and store nothing)
    const int r = i >> 6, x = i & (MLT_MC_TILE_W - 1);
    int32_t t = 0;
    if (x < w) {
#pragma unroll
      for (int k = 0; k < 8; ++k) t += cx[k] * (int32_t)win[r * MLT_MC_WIN_PITCH + x + k];
    }
    hor[i] = t;
  }
  __syncthreads();

  for (int i = tid; i < h * (MLT_MC_TILE_W / 8); i += 256) {
    const int y = i >> 3, seg = i & 7, x = 8 * seg;
    if (x >= w) continue;
    int32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int32_t *row = hor + (y + j) * MLT_MC_TILE_W + x;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += cy[j] * row[e];
    }
    uint32_t o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (uint32_t)motion_clampi((v[e] + 2048) >> 12, 0, 1023);
    int16_t *d = a.dst + (size_t)(ty0 + y) * (size_t)a.dst_pitch + tx0 + x;
    if (a.vec_dst && x + 8 <= w) {
      pic_u32x4 q;
      q.x = o[0] | (o[1] << 16); q.y = o[2] | (o[3] << 16); q.z = o[4] | (o[5] << 16); q.w = o[6] | (o[7] << 16);
      *(pic_u32x4 *)d = q;
    } else {
      for (int e = 0; e < 8 && x + e < w; ++e) d[e] = (int16_t)o[e];
    }
  }
}

// ---- motion_refine_kernel: one workgroup (256 lanes) per block; quarter-sample refinement of every reference's integer winner and the choice among them ----
// (include/mltcnn.h: mlt_picture_predict_refs.)  For reference r with integer winner (dx, dy) (the search's field, slice r: {4 dx, 4 dy}) the candidates are
// mv = (4 dx + qx, 4 dy + qy), qx, qy in {-w, -w + step, ..., w}: (w, step) = (0, 1), (2, 2), (3, 1) for subpel 0, 1, 2 -- nq = 1, 3 or 7 values a side.
// mv >> 2 = d + (q >> 2) in {d - 1, d} and mv & 3 = q & 3, so everything a candidate reads lies in offsets -4 .. bw + 3 of the integer winner's position.
// LDS (dynamic, mlt_motion_refine_lds(B)): the clamped window win[B + 8][B + 8] int16, sample (r, c) = R(x0 + dx - 4 + c, y0 + dy - 4 + r), rows < bh + 8 and
// columns < bw + 8 staged; the block cur[B][B] int16 (rows < bh, columns < bw staged); ONE fraction's horizontal pass hor[B + 8][B] int32, hor[rr][x] =
// sum_k C[qx & 3][k] win[rr][x + (qx >> 2) + k + 1]; the four waves' partial sums [4][7] uint32.
// Per qx: the horizontal pass; then lane t takes the samples t, t + 256, ... of the block and runs the vertical pass of ALL nq fractions qy on each (nine rows of
// hor per sample, eight of them per fraction: row y + (qy >> 2) + j + 1 for tap j), clip and |cur - P| into nq running sums; a wave reduction by shuffles and the
// four waves' sums through LDS give SADP of the nq candidates, and lane 0 keeps the smallest 64-bit key  cost_q << 32 | l1 << 22 | r << 20 | (mvy + 512) << 10 |
// (mvx + 512)  over every (r, qx, qy): ONE unsigned compare states the order (cost_q, l1, r, mvy, mvx), so no evaluation order matters.  No atomics.
// cost_q = 4 SADP + lambda (|mvx| + |mvy|) <= 4 x 4096 x 33791 + 65535 x 518 < 2^32.  Lane 0 writes the block's vector, cost_q and reference index.
#define MLT_REFINE_MAX_Q 7

__global__ __launch_bounds__(256) void motion_refine_kernel(const MotionRefineArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int B = 1 << a.block_l, Wp = B + 8;
  int32_t *hor = (int32_t *)smem;                        // [Wp][B]
  uint32_t *wsum = (uint32_t *)(hor + Wp * B);           // [4][MLT_REFINE_MAX_Q]
  int16_t *win = (int16_t *)(wsum + 4 * MLT_REFINE_MAX_Q + 4);   // [Wp][Wp]
  int16_t *cur = win + Wp * Wp;                          // [B][B]
  const int x0 = (int)blockIdx.x << a.block_l, y0 = (int)blockIdx.y << a.block_l;
  const int bw = min(B, a.width - x0), bh = min(B, a.height - y0);
  const int tid = threadIdx.x;
  const size_t blk = (size_t)blockIdx.y * (size_t)a.bx + blockIdx.x;
  const int qw = a.subpel == 2 ? 3 : (a.subpel == 1 ? 2 : 0), qstep = a.subpel == 1 ? 2 : 1, nq = a.subpel == 2 ? 7 : (a.subpel == 1 ? 3 : 1);

  for (int i = tid; i < bh * B; i += 256) {
    const int r = i >> a.block_l, c = i & (B - 1);
    if (c < bw) cur[i] = a.cur[(size_t)(y0 + r) * (size_t)a.cur_pitch + (x0 + c)];
  }

  int cy[MLT_REFINE_MAX_Q][8];   // the vertical taps of the nq fractions (uniform)
#pragma unroll
  for (int q = 0; q < MLT_REFINE_MAX_Q; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) cy[q][j] = kMotionTaps[((q < nq ? q : 0) * qstep - qw) & 3][j];

  unsigned long long best = ~0ull;   // lane 0's
  for (int r = 0; r < a.n_refs; ++r) {
    const int16_t *ref = r == 0 ? a.refs[0] : (r == 1 ? a.refs[1] : (r == 2 ? a.refs[2] : a.refs[3]));
    const long ref_pitch = r == 0 ? a.ref_pitches[0] : (r == 1 ? a.ref_pitches[1] : (r == 2 ? a.ref_pitches[2] : a.ref_pitches[3]));
    const int16_t *mv0 = a.mv_int + (size_t)r * a.mv_int_slice + 2 * blk;
    const int dx = (int)mv0[0] >> 2, dy = (int)mv0[1] >> 2;   // the search's vectors are multiples of 4
    const int ww = bw + 8, wh = bh + 8;
    __syncthreads();   // the previous reference's last horizontal pass has read win
    for (int i = tid; i < ww * wh; i += 256) {
      const int rr = i / ww, c = i - rr * ww;
      const int gx = motion_clampi(x0 + dx - 4 + c, 0, a.width - 1), gy = motion_clampi(y0 + dy - 4 + rr, 0, a.height - 1);
      win[rr * Wp + c] = ref[(size_t)gy * (size_t)ref_pitch + gx];
    }
    __syncthreads();

    for (int qxi = 0; qxi < nq; ++qxi) {
      const int qx = qxi * qstep - qw, ixo = qx >> 2, fx = qx & 3;
      int cx[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) cx[k] = kMotionTaps[fx][k];
      for (int i = tid; i < wh * B; i += 256) {
        const int rr = i >> a.block_l, x = i & (B - 1);
        if (x < bw) {
          const int16_t *w = win + rr * Wp + x + ixo + 1;
          int32_t t = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) t += cx[k] * (int32_t)w[k];
          hor[i] = t;
        }
      }
      __syncthreads();

      uint32_t sad[MLT_REFINE_MAX_Q];
#pragma unroll
      for (int q = 0; q < MLT_REFINE_MAX_Q; ++q) sad[q] = 0;
      for (int i = tid; i < bh * B; i += 256) {
        const int y = i >> a.block_l, x = i & (B - 1);
        if (x >= bw) continue;
        int32_t t[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) t[j] = hor[(y + j) * B + x];
        const int c = cur[i];
#pragma unroll
        for (int q = 0; q < MLT_REFINE_MAX_Q; ++q) {
          if (q < nq) {
            const int qy = q * qstep - qw;
            int32_t v = 0;
            if (qy < 0) {
#pragma unroll
              for (int j = 0; j < 8; ++j) v += cy[q][j] * t[j];
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j) v += cy[q][j] * t[j + 1];
            }
            const int p = motion_clampi((v + 2048) >> 12, 0, 1023);
            sad[q] += (uint32_t)abs(c - p);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < MLT_REFINE_MAX_Q; ++q) {
        for (int off = 32; off > 0; off >>= 1) sad[q] += __shfl_xor(sad[q], off, 64);
        if ((tid & 63) == 0) wsum[(tid >> 6) * MLT_REFINE_MAX_Q + q] = sad[q];
      }
      __syncthreads();   // and every lane has read hor
      if (tid == 0) {
        const int mvx = 4 * dx + qx;
        for (int q = 0; q < nq; ++q) {
          const uint32_t s = wsum[q] + wsum[MLT_REFINE_MAX_Q + q] + wsum[2 * MLT_REFINE_MAX_Q + q] + wsum[3 * MLT_REFINE_MAX_Q + q];
          const int mvy = 4 * dy + q * qstep - qw;
          const uint32_t l1 = (uint32_t)(abs(mvx) + abs(mvy));
          const uint32_t cost = 4u * s + (uint32_t)a.lambda * l1;
          const unsigned long long key = ((unsigned long long)cost << 32) | ((unsigned long long)l1 << 22) | ((unsigned long long)r << 20) |
                                         ((unsigned long long)(mvy + 512) << 10) | (unsigned long long)(mvx + 512);
          best = key < best ? key : best;
        }
      }
      // (lane 0 reads wsum before it reaches the next barrier, and wsum is written again only behind that barrier)
    }
  }
  if (tid == 0) {
    const int mvx = (int)(best & 0x3ff) - 512, mvy = (int)((best >> 10) & 0x3ff) - 512;
    *(uint32_t *)(a.mv + 2 * blk) = (uint32_t)(uint16_t)(int16_t)mvx | ((uint32_t)(uint16_t)(int16_t)mvy << 16);
    a.cost[blk] = (uint32_t)(best >> 32);
    a.ref_out[blk] = (uint8_t)((best >> 20) & 3);
  }
}
