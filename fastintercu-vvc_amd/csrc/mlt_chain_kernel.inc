// mlt_chain_kernel.inc -- chain_kernel: the BasicBlock tail of a stage / a whole stage in one launch; part of mlt_kernels.hip (one translation unit).
// A kernel argument re-read from the kernarg segment AT THE POINT OF USE (one s_load, base pointer made opaque): for pointers that are
// needed once per tile in a kernel whose scalar registers are exhausted -- kept live they are spilled to a VGPR lane and from there to
// scratch, and every scratch reload costs a round trip plus an s_waitcnt vmcnt(0) that drains the LDS-DMA in flight.
template <class T> __device__ __forceinline__ T karg_reload(size_t off) {
  const __attribute__((address_space(4))) char *ka = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  return *(const __attribute__((address_space(4))) T *)(ka + off);
}
#define KARG(type, member) karg_reload<type>(offsetof(ChainArgs, member))

// ---------------------------------------------------------------------------------------------
// Fused chain of stride-1 3x3 convs on WHOLE samples (the BasicBlock tail of the 128@16 stage, arch:52-57):
//     b0 = relu(bn2(conv2(t)) + sc) ;  t1 = relu(bn1(conv1(b0))) ;  out = relu(bn2(conv2(t1)) + b0)  (+ GAP, arch:288)
// One 16-wave workgroup owns one sample: the 16 x 16 x 128 activation (64 KiB fp16) lives in LDS for the whole chain,
// every conv reads it from there and its epilogue writes the next activation back IN PLACE (all waves have passed the
// last weight step's barrier, so nobody reads the buffer any more); b0 -- the residual of the last conv -- stays in the
// registers of the wave that produced it (a wave's output tile covers the same pixels x channels in every conv).  HBM
// sees t and sc in, out (or only the GAP sums) out: no intermediate is written or re-read, no patch is staged per
// conv, and three launches become one.
//   * no halo: a tile is a whole sample, so a tap that leaves the map is conv padding.  Such a lane reads an address beyond the
//     workgroup's LDS allocation, which returns zeros on gfx950 (OOBZ; probed at mlt_init, which selects the masked form of the kernel otherwise) -- the earlier form, the
//     lane's own pixel ANDed with a zero mask, cost 8 VALU ops per k-step in the loop where issue slots are scarce (4-6 %);
//     the buffer is unpadded, 16-byte channel slots XOR-swizzled with the pixel index (conflict-free ds_read_b128 for
//     16 consecutive pixels, as in the LDS-DMA kernels above);
//   * weights stream through the same LDS-DMA ring as conv_ring_dma_kernel (first half of the waves), continuously
//     across convs and samples; 64 KiB activation + 2 x 48 KiB ring = the whole 160 KiB;
//   * the next sample's input is fetched by LDS-DMA (second half of the waves) into each 64-channel region of the buffer
//     as soon as the LAST conv has finished reading it: region c during chunk c+1, the last region during the final
//     epilogue and the next sample's first chunk.
// Bit-identical to the three stand-alone launches (same k order, same rounding points: fp16 activations between convs).
// ---------------------------------------------------------------------------------------------
//   * C = 256 (8 x 8 maps, two samples per workgroup): the couts are computed in NPASS = 2 passes of 128 (the stand-alone
//     layer's weight packing); a pass cannot overwrite the buffer while the other still reads it, so pass 0 holds its
//     activated tile in registers (16 VGPRs) until pass 1 has finished.
//   * S2 (whole stage in one launch): the stage's first conv -- 3x3 stride 2 (+ bn1 + ReLU) and its 1x1 stride-2 projection
//     shortcut (+ BN), arch:44-55 -- runs in front of the chain ON THE SAME TILE: its input (C/2 channels at 2H x 2H) is staged
//     16 channels at a time as a zero-padded, column-parity-split patch ((2H+1)^2 pixels x 32 B, slot-swizzled by bit 3 of the
//     pixel index) into the then idle activation buffer, double-buffered; 10 weight "taps" (9 + shortcut) of a chunk are one
//     40 KiB ring step.  t goes straight into the activation buffer, sc into the residual registers: neither touches HBM.
//     LDS during this phase: patches [0, 2 x PBYTES), ring steps at ACT + 8 KiB and ACT + WCHUNK + 8 KiB -- chosen so that
//     the first chain step can be prefetched during the last stride-2 step and vice versa (see the hazards at issue_ring).
//   * KEEP = false (64 channels @ 32 x 32: a whole sample is 128 KiB, weights stream 1 tap = 8 KiB per step through a 4-deep ring,
//     a wave owns 64 couts x 128 pixels = 8 accumulators = 128 VGPRs): no room to keep b0 in registers -- conv 0 also writes it
//     to HBM (ChainConv.y) and the last conv reads it back (L2-hot) as an ordinary residual, both loaded AFTER the last step's
//     MFMA loop.  One channel chunk only, so the next sample's input can be fetched only after the last step of the last conv.
//   * W2 (hi+lo-WEIGHTS tier, round 4): every ring step carries TWO weight planes (hi, lo; fast tiling, mlt_model.cpp MLT_MODEL_W2) and every
//     (tap, k-step) item runs Wh * X then Wl * X on the same activation fragment: 2 MFMAs per product, 1.5x the fragment reads, twice the
//     ring bytes per tap -- so one tap per step (GT = 1) through a 3-deep ring (stages) / 2-deep ring (64-channel chain).  Per accumulator
//     the order is (chunk, tap, k-step, hi, lo): the order of conv_mfma_kernel<NSPLIT = 3> on the same packing, which serves small launches.
//     No stride-2 front conv in this form (its 10-tap steps fill the LDS with one plane): the stage's first conv stays a launch of its own.
//   * LO8 (with W2): the lo plane is FP8 and the lo product of a (tap, chunk) ONE v_mfma_scale_f32_32x32x64_f8f6f4 at twice the fp16 rate (see
//     cvt_frag_fp8 / mfma_lo8 in mlt_kernels.hip): a ring step carries the hi plane + half as many lo bytes.  Its B operand comes from an
//     E4M3 IMAGE of the activation kept in LDS next to the fp16 one (32 KiB: [region][pixel][64 B], 16-byte slots swizzled with the pixel
//     index), written by the same epilogue that writes the fp16 activation (and, for the tile's DMA'd input, by one conversion pass at the
//     tile top): every activation is converted ONCE per conv.  (First form of this kernel: each item converted its fp16 fragment in
//     registers -- v_cvt_scalef32_pk_fp8_f16 nine times per activation -- and the conversions ate the whole gain: 1.57 ms against 1.26 with
//     them knocked out.)  Per accumulator: hi k-steps 0..3 of a tap, then its lo product.
//   * WIDE (stage256_wide_kernel: the whole 256-channel stage, two cout passes): a wave carries the accumulators of BOTH cout passes -- its two 32-cout
//     blocks in pass 0 and in pass 1, 128 couts x 32 pixels -- so one activation fragment feeds four MFMAs instead of two being read once per pass
//     (fragment reads per two MFMAs 3 -> 2.5), and every stride-2 input patch is staged ONCE per tile instead of once per pass.  Ring steps keep
//     their bytes, their number and their MFMAs per wave, cut the other way:
//       stride-1 convs: a step is 6 consecutive (tap, k16) items of a 64-channel chunk for both passes -- two contiguous 24 KiB runs of the packing
//         [pass][chunk][tap][k16][4 blocks][1 KiB] -- 6 steps per chunk, 24 per conv; every second step starts in the middle of a tap, and a step PAIR
//         (12 items = 3 taps) is unrolled statically;
//       stride-2 phase: a step is taps 0-4 or taps 5-9 (the shortcut tap included) of a 16-channel chunk for both passes -- two contiguous 20 KiB
//         runs of s2_w; patch c serves steps 2c and 2c + 1 (8 patch DMAs per tile instead of 16), three patch buffers, patch c in buffer c % 3,
//         requested at step 2c - 4.
//     Per accumulator the order is still (chunk, tap, k16): every logit keeps its bytes.  Both passes end together, so no tile is held back in
//     registers (hold0 / hold) while the other pass still reads the buffer.
template <int C, int HL, int SPW_L, int WCB, int WPB, int WAVES_C, int WAVES_P, int GT, int RB, int FD, int MINW, int NCONV, bool SPLIT_ROLES, bool S2 = false, bool KEEP = true, bool OOBZ = false, bool W2 = false, bool LO8 = false, bool WIDE = false>
__device__ __forceinline__ void chain_body(const ChainArgs &a) {
  constexpr int KC = 64, NCHUNK = C / KC, KS = KC / 16, SLOTS = KC / 8, TAPS = 9, NG = (TAPS + GT - 1) / GT, GT_LAST = TAPS - (NG - 1) * GT;  // a last, shorter tap group when GT does not divide 9
  constexpr int CBT = WCB * WAVES_C, CT = 32 * CBT, NPASS = C / CT, NW = WAVES_C * WAVES_P;
  constexpr int H = 1 << HL, HW = H * H, M = HW << SPW_L;
  static_assert(C % CT == 0 && NPASS <= 2 && M == 32 * WAVES_P * WPB && HW >= 32 && C % KC == 0, "tiling");
  static_assert(NCONV == 3, "the chain is a stage's three stride-1 convs (mlt_launch_chain launches no other)");
  static_assert(GT_LAST == GT || RB == 2, "a shorter last tap group issues fewer ring pieces: only with the uncounted vmcnt(0) wait of a 2-deep ring");
  constexpr int WP = (W2 && !LO8) ? 2 : 1, WPLANE = GT * KS * CBT * 1024;  // fp16 weight planes per step, bytes of one plane of a step
  constexpr int WLO8 = LO8 ? GT * CBT * 2048 : 0;                           // FP8 lo plane of a step: 2 KiB per (tap, 32-cout block)
  constexpr int WCHUNK = WP * WPLANE + WLO8, NPIECE = WCHUNK / 1024, NBUF = RB, PFD = RB - 1;
  static_assert(!W2 || (!S2 && GT_LAST == GT), "hi+lo weights: no stride-2 front conv, whole tap groups");
  static_assert(!LO8 || (W2 && KS == 4 && FD == 1 && KEEP && NCHUNK > 1), "FP8 lo plane: 64-channel chunks, fragment reads one item ahead, stage forms");
  constexpr int REGION8 = LO8 ? M * KC : 0, ACT8 = NCHUNK * REGION8;  // LO8: the e4m3 image of the activation, behind the weight ring
  // SPLIT_ROLES: first half of the waves issues the ring DMA (and waits for it every step), second half the activation DMA;
  // otherwise every wave issues its share of both and waits for everything it issued at the end of a step
  constexpr int NWR = SPLIT_ROLES ? NW / 2 : NW, NWP = SPLIT_ROLES ? NW - NWR : NW, WP0 = SPLIT_ROLES ? NWR : 0;
  constexpr int PPWR = (NPIECE + NWR - 1) / NWR;
  constexpr int REGION = M * KC * 2, ACT = NCHUNK * REGION, RPIECE = REGION / 1024, PPR = (RPIECE + NWP - 1) / NWP;
  constexpr int A8BASE = ACT + NBUF * WCHUNK;
  static_assert(A8BASE + ACT8 <= 160 * 1024, "LDS");
  static_assert(RB >= 2 && RB <= 4, "ring depth");
  static_assert(SPLIT_ROLES || RB == 2, "unified issue waits with vmcnt(0)");
  static_assert(!S2 || KEEP, "the whole-stage variant keeps sc / b0 in registers");
  static_assert(FD >= 1 && FD <= 3 && FD * (WP * WCB + WPB) + (LO8 ? 2 * (WCB > WPB ? WCB : WPB) : 0) <= 15, "fragment prefetch distance");
  static_assert((WP - 1) * WPLANE + ((GT * KS - 1) * CBT + WCB - 1) * 1024 < 65536 && WPLANE + WLO8 < 65536, "fragment offsets are ds_read immediates");
  // stride-2 front conv (S2)
  constexpr int CIN = C / 2, HIN = 2 * H, KCS = 16, NCS = CIN / KCS, TAPS_S = 10, NS = S2 ? NPASS * NCS : 0;
  constexpr int NCH = NCONV * NPASS * NCHUNK * NG;                       // chain steps per tile
  constexpr int WSTEP_S = TAPS_S * CBT * 1024, NPIECE_S = WSTEP_S / 1024;
  constexpr int PRS = 2 * H + 1, PCW = 2 * H + 1, PPS = PRS * PCW, PPIX = PPS << SPW_L;  // patch rows, columns (H+1 odd + H even), pixels
  constexpr int PBYTES = (PPIX * KCS * 2 + 1023) / 1024 * 1024, PPIECE = PBYTES / 1024;
  constexpr int SOFF0 = ACT + 8 * 1024, SOFF1 = ACT + WCHUNK + 8 * 1024;  // LDS offsets of the two stride-2 weight steps
  // patch buffers: three where they fit below the first weight step (8 x 8 maps: 19 KiB patches) -> a patch is requested two steps
  // before it is read; else two.  Either way the LAST step of a tile reads buffer 0, the only one the first chain step's weights
  // (landing in [ACT, ACT + WCHUNK) meanwhile) cannot overlap.
  constexpr int NPB = 3 * PBYTES <= SOFF0 ? 3 : 2, PLA = NPB - 1;
  auto pbuf = [](int i) { return NPB == 3 ? i % 3 : (i + 1) & 1; };
  static_assert(!S2 || WIDE || (NPB == 3 ? (NS - 1) % 3 == 0 : (NS - 1) % 2 == 1), "S2: the last stride-2 step must read patch buffer 0");
  // WIDE: items of a stride-1 step, taps of a stride-2 step, LDS distance of the two passes' runs inside a step of either kind
  constexpr int WI = 6, NG6 = TAPS * KS / WI, WHALF = WCHUNK / 2, TH = TAPS_S / 2, WHALF_S = WSTEP_S / 2;
  static_assert(!WIDE || (NPASS == 2 && S2 && KEEP && OOBZ && !W2 && NCONV == 3 && GT == 3 && KS == 4 && FD == 1 && 2 * WI == GT * KS && NG6 * WI == TAPS * KS),
                "WIDE: the whole 256-channel stage, conv padding from beyond the LDS, fragment reads one item ahead");
  // (the last stride-2 step reads buffer (NCS - 1) % 3 while the first chain step's weights land in [ACT, ACT + WCHUNK): no patch buffer reaches that far)
  static_assert(!WIDE || (NPB == 3 && NCS >= 3 && 3 * PBYTES <= ACT), "WIDE: three patch buffers, all below the chain's ring slot 0");
  static_assert(!WIDE || (WHALF + ((WI - 1) * CBT + WCB - 1) * 1024 < 65536 && WHALF_S + ((TH - 1) * CBT + WCB - 1) * 1024 < 65536), "WIDE: fragment offsets are ds_read immediates");
  static_assert(!S2 || (SPLIT_ROLES && RB == 2 && NS % 2 == 0 && NCH % 2 == 0 && (NCS - 1) % 2 == 1), "S2: step parities");
  static_assert(!S2 || (2 * PBYTES <= SOFF0 && SOFF0 + WSTEP_S <= ACT + WCHUNK && SOFF1 + WSTEP_S <= 160 * 1024), "S2: LDS layout");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *ring = smem + ACT;
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave % WAVES_C, wp = wave / WAVES_C;
  const int p = lane & 31, h = lane >> 5;
  const bool ring_wave = wave < NWR, patch_wave = wave >= WP0;
  const int lane16 = lane * 16;

  // lane -> pixels: EXACTLY the map of the stand-alone kernels (lane ranking; on 8-wide maps a 16-lane ds_read_b128 group
  // owns rows a and a + 4 of a sample), so that the fp32 GAP butterfly adds the same pixels in the same order and the
  // logits are bit-identical whichever kernel variant serves a batch.  mj: logical position (GAP slot), pj: pixel
  // (sample, y, x) = its LDS slot.
  const int pr = p < 4 ? p : p < 12 ? p + 12 : p < 16 ? p - 8 : p < 20 ? p + 8 : p < 28 ? p - 12 : p;
  int mj[WPB], pj[WPB];
#pragma unroll
  for (int j = 0; j < WPB; ++j) {
    mj[j] = (wp * WPB + j) * 32 + pr;
    if constexpr (HL == 3) {
      const int q = mj[j] >> 3, k = q & 7;
      pj[j] = ((q & ~7) | ((k & 1) << 2) | (k >> 1)) * 8 + (mj[j] & 7);
    } else pj[j] = mj[j];
  }
  // maps wider than 8: a lane's pixel blocks are 32 pixels apart and position == pixel, so ONE register carries all of them (the
  // opaque copies that keep address terms from being hoisted would otherwise pin 2 * WPB registers: the 64-channel chain is at the cap)
  auto opaque_pixels = [&]() {
    if constexpr (HL != 3 && WPB > 1) {
#pragma unroll
      for (int j = 1; j < WPB; ++j) { pj[j] = pj[0] + 32 * j; mj[j] = pj[j]; }
      mj[0] = pj[0];
    }
  };
  // 16-byte channel slot swizzle of pixel q: two pixels share a 256-byte bank row; on 8-wide maps bit 5 of q (row a vs
  // a + 4) is folded in so that the two rows of a lane group use disjoint columns
  // (16-wide maps: bit 4 of q -- the row parity -- is folded in as well, so that the epilogue's ds_write_b128, whose 8-lane groups
  // cover columns 0-3 of two consecutive rows, is conflict-free too)
#ifndef CFG_CHAIN_SWZ16
#define CFG_CHAIN_SWZ16 1
#endif
  // OOBZ: a tap outside the map reads an LDS address beyond the allocation (DS reads out of range return 0 on gfx950) instead of the
  // lane's own pixel ANDed with a zero mask (8 VALU ops per k-step and wave: knock-out -4..6 % per launch).  Both forms are built for the
  // three kernels of the default path; the context picks per device (mlt_probe_lds_oob at mlt_init).
#ifndef CFG_CHAIN_SWZ32  // 32-wide maps: 0 = no extra bit.  A read window of a dx = +-1 tap crosses a 16-pixel boundary there, and any
#define CFG_CHAIN_SWZ32 0  // term that depends on bit 4 of q then maps two same-parity pixels of the window to one slot (2-way conflict on 6 of 9 taps)
#endif
  auto swz = [](int q) {
    return ((q >> 1) & (SLOTS - 1)) ^ (HL == 3 ? ((q >> 5) & 1) << 2 : HL == 4 ? (CFG_CHAIN_SWZ16 ? ((q >> 4) & 1) << 1 : 0) : (CFG_CHAIN_SWZ32 ? ((q >> 4) & 1) << 1 : 0));
  };

  const int ntiles = (a.n + (1 << SPW_L) - 1) >> SPW_L;
  int t = blockIdx.x;
  const int tstep = gridDim.x;
  if (t >= ntiles) return;

  // ---- weight ring: one global step sequence (sample, [stride-2: cout pass, chunk], conv, cout pass, chunk, tap group) ----
  // S2 hazards (step i+1 is DMA'd while step i computes; steps of both kinds alternate slots from 0 in every tile):
  //   last chain step (reads chain slot 1 = [ACT+WCHUNK, ..)) -> next tile's first stride-2 step lands in SOFF0 (inside chain slot 0: free);
  //   last stride-2 step (odd index: reads SOFF1 and patch buffer 0) -> first chain step lands in chain slot 0 = [ACT, ACT+WCHUNK):
  //   overlaps only patch buffer 1's tail and SOFF0, both last read one step earlier.
  int steps_to_issue = ((ntiles - 1 - t) / tstep + 1) * (NS + NCH);
  int r_pos = 0, r_cv = 0, r_ps = 0, r_ci = 0, r_gi = 0, ahead = 0;  // r_pos: position in the tile's NS + NCH steps
  int slot_wr = 0;  // ring slot of the next chain step (S2: NCH is even and RB == 2, so every tile starts at slot 0 again)
  auto issue_ring = [&]() {
    if (steps_to_issue <= 0) return;
    const bool s_step = S2 && r_pos < NS;
    if (ring_wave) {
      if (s_step) {
      } else if constexpr (WIDE) {  // items [WI * r_gi, WI * r_gi + WI) of chunk r_ci, pass 0 then pass 1: NPIECE / 2 pieces each
        const char *wsrc = (const char *)(r_cv == 0 ? a.cv[0].w : r_cv == 1 ? a.cv[1].w : a.cv[2].w);
        char *dst = ring + slot_wr * WCHUNK;
#pragma unroll
        for (int k = 0; k < PPWR; ++k) {
          const int pi = wave + k * NWR, ps = pi / (NPIECE / 2), pw = pi - ps * (NPIECE / 2);
          static_assert(!WIDE || NPIECE % NWR == 0, "every ring wave issues PPWR pieces");
          glds16(wsrc + (size_t)((ps * NCHUNK + r_ci) * (TAPS * KS) + r_gi * WI) * (CBT * 1024) + pw * 1024 + lane16, dst + pi * 1024);
        }
      } else {
        const char *wsrc = (const char *)(r_cv == 0 ? a.cv[0].w : r_cv == 1 ? a.cv[1].w : a.cv[2].w);
        const char *src = wsrc + (size_t)((r_ps * NCHUNK + r_ci) * TAPS + r_gi * GT) * (KS * CBT * 1024);
        char *dst = ring + slot_wr * WCHUNK;
        const int npiece = (GT_LAST != GT && r_gi == NG - 1) ? GT_LAST * KS * CBT : NPIECE;  // (never read behind the layer's last tap)
        const size_t wlo = W2 ? (r_cv == 0 ? a.cv[0].w_lo_off : r_cv == 1 ? a.cv[1].w_lo_off : a.cv[2].w_lo_off) : 0;
#pragma unroll
        for (int k = 0; k < PPWR; ++k) {
          int pi = wave + k * NWR;
          pi = pi < npiece ? pi : npiece - 1;  // every ring wave issues exactly PPWR instructions per step (counted vmcnt)
          // W2: pieces [0, WPLANE / 1024) are the hi plane of the step, the rest the lo plane (same offsets behind w_lo_off; LO8: the FP8
          // plane, 2 KiB per (tap, 32-cout block), contiguous over the taps of the step)
          const int pl = W2 ? pi / (WPLANE / 1024) : 0, pw = W2 ? pi - pl * (WPLANE / 1024) : pi;
          if (LO8 && pl) glds16(wsrc + wlo + (size_t)((r_ps * NCHUNK + r_ci) * TAPS + r_gi * GT) * (CBT * 2048) + pw * 1024 + lane16, dst + pi * 1024);
          else glds16(src + (pl ? wlo : 0) + pw * 1024 + lane16, dst + pi * 1024);
        }
      }
    }
    if (s_step) {  // stride-2 weight steps: every wave issues its share (all waves wait with vmcnt(0) at the end of those steps anyway)
      const char *src = (const char *)a.s2_w + (size_t)r_pos * WSTEP_S;
      char *dst = smem + ((r_pos & 1) ? SOFF1 : SOFF0);
#pragma unroll
      for (int k = 0; k < (NPIECE_S + NW - 1) / NW; ++k) {
        const int pi = wave + k * NW;
        if constexpr (WIDE) {  // step r_pos = (chunk r_pos / 2, taps 0-4 | taps 5-9), pass 0 then pass 1: NPIECE_S / 2 pieces each
          const int ps = pi / (NPIECE_S / 2), pw = pi - ps * (NPIECE_S / 2);
          const char *srcw = (const char *)a.s2_w + (size_t)((ps * NCS + (r_pos >> 1)) * TAPS_S + (r_pos & 1) * TH) * (CBT * 1024);
          if (pi < NPIECE_S) glds16(srcw + pw * 1024 + lane16, dst + pi * 1024);
        } else if (pi < NPIECE_S) glds16(src + pi * 1024 + lane16, dst + pi * 1024);
      }
    }
    --steps_to_issue;
    ++ahead;
    if (!s_step) {
      if (++slot_wr == NBUF) slot_wr = 0;
      if constexpr (WIDE) {
        if (++r_gi == NG6) { r_gi = 0; if (++r_ci == NCHUNK) { r_ci = 0; if (++r_cv == NCONV) r_cv = 0; } }
      } else if (++r_gi == NG) { r_gi = 0; if (++r_ci == NCHUNK) { r_ci = 0; if (++r_ps == NPASS) { r_ps = 0; if (++r_cv == NCONV) r_cv = 0; } } }
    }
    if (++r_pos == NS + NCH) r_pos = 0;
  };
  // ---- S2: input patch of stride-2 step i (16 channels, chunk i % NCS) -> patch buffer (i + 1) & 1 (patch waves).  Patch pixel
  // qS = (sample * PRS + r) * PCW + k holds input pixel (r - 1, k <= H ? 2k - 1 : 2(k - H - 1)); its two 16-byte channel slots are
  // swapped when bit 3 of qS is set (16 consecutive patch pixels span two 256-byte bank rows).  Outside the picture: zero page.
  // Addressing: everything that depends only on (lane, piece) is packed ONCE into 32 bits per piece -- byte offset inside the
  // (sample, 16-channel chunk) | sample-in-tile << 30 | "outside the picture" << 31 -- and the 64-bit source address is formed at the
  // point of issue from an opaque copy.  Left to itself the compiler precomputes the 64-bit addresses of all pieces at the top of a
  // tile, runs out of registers, and reloads them from scratch BETWEEN the DMA instructions: every reload is followed by
  // s_waitcnt vmcnt(0), i.e. by a full round trip of the piece just requested (seen in the ISA: 280 B of scratch, 3 serialised round
  // trips per stride-2 step and 5 in front of the last epilogue's stores).
  constexpr int PPW = (PPIECE + NW - 1) / NW;
  uint32_t pvo[S2 ? PPW : 1];
  if constexpr (S2) {
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
      const int piece = wave + k * NW;
      const int it = piece * 64 + lane, qS = it >> 1, pos = it & 1;
      const int sl = pos ^ ((qS >> 3) & 1);
      const int sm = qS / PPS, rem = qS - sm * PPS, r = rem / PCW, kk = rem - r * PCW;
      const int ri = r - 1, ci = kk <= H ? 2 * kk - 1 : 2 * (kk - H - 1);
      const bool live = qS < PPIX && ri >= 0 && ri < HIN && ci >= 0 && ci < HIN;
      const uint32_t off = a.x_c16 ? ((ri * HIN + ci) * KCS + sl * 8) * 2   // [n][CIN/16][HIN*HIN][16]
                                   : ((ri * HIN + ci) * CIN + sl * 8) * 2;  // NHWC
      pvo[k] = live ? off | ((uint32_t)sm << 30) : 0x80000000u;
    }
  }
  const uint32_t chunk_stride = a.x_c16 ? HIN * HIN * KCS * 2 : KCS * 2;
  auto patch_dma = [&](int tile, int i) {  // every wave issues its share
    const int chunk = i % NCS;
    char *dst = smem + pbuf(i) * PBYTES;
    const char *xb = (const char *)a.x + (size_t)chunk * chunk_stride;
    uint32_t zo = ((int)blockIdx.x * 64 * NW + tid) * 16;
    asm volatile("" : "+v"(zo));
    const char *zsrc = (const char *)a.zero + (zo & 0xFFF0);
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
      const int piece = wave + k * NW;
      if (piece >= PPIECE) break;  // wave-uniform
      uint32_t v = pvo[k];
      asm volatile("" : "+v"(v));
      int n = (tile << SPW_L) + (int)((v >> 30) & 1);
      n = n < a.n ? n : a.n - 1;
      const char *src = (int)v < 0 ? zsrc : xb + (size_t)n * (size_t)(CIN * HIN * HIN * 2) + (v & 0x3FFFFFFFu);
      glds16(src, dst + piece * 1024);
    }
  };
  // ---- activation regions (patch waves): item it = (pixel q, position pos) at byte it * 16 of the region holds channel slot
  // pos ^ ((q >> 1) & 7) of that pixel ----
  auto dma_region = [&](int tile, int c) {
    if (!patch_wave) return;
    // per-piece source offsets are formed here (a few bit operations) from a rematerialised lane id, not hoisted and kept live
    int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int k = 0; k < PPR; ++k) {
      const int piece = (wave - WP0) + k * NWP;
      if (piece >= RPIECE) break;  // wave-uniform
      const int it = piece * 64 + ln, q = it / SLOTS, pos = it & (SLOTS - 1);
      const int sl = pos ^ swz(q);
      int n = (tile << SPW_L) + (q >> (2 * HL));
      n = n < a.n ? n : a.n - 1;  // ragged last tile: a valid sample again (its outputs are masked)
      // (NHWC only.  A chunk-major t for the 64-channel chain was tried: its writer's stores gain what this DMA -- four slots of a pixel per
      // lane quad = two cache lines instead of one -- loses, and the second address form cost this loop a scratch reload per piece)
      const char *src = (const char *)a.x + (((size_t)n * HW + (q & (HW - 1))) * C + c * KC + sl * 8) * 2;
      glds16(src, smem + c * REGION + piece * 1024);
    }
  };

  // ---- prologue ----
  if constexpr (S2) {
#pragma unroll
    for (int i = 0; i < NPB; ++i) patch_dma(t, i);
  } else {
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) dma_region(t, c);
  }
#pragma unroll
  for (int d = 0; d < PFD; ++d) issue_ring();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");

  int slot_rd = 0;
  PHC_DECL;
  // Biases live in registers for the life of the (persistent) workgroup: lane l holds the bias of cout (wc * WCB) * 32 + l of every
  // conv and cout pass (5 VGPRs for the 128 stage, 10 for the 256 stage); an epilogue fetches the 16 values of its accumulator rows
  // with ds_bpermute (crossbar only, no LDS memory).  A bias LOADED in an epilogue costs an exposed L2 round trip four times per
  // tile, and the compiler's s_waitcnt vmcnt(0) in front of its first use also waits for whatever LDS-DMA was issued before it --
  // in the last epilogue that is the next tile's complete input patch.
  constexpr bool PBIAS = WCB == 2;
  float pb_cv[NCONV][NPASS], pb_t[NPASS], pb_sc[NPASS];
  if constexpr (PBIAS) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
#pragma unroll
      for (int c = 0; c < NCONV; ++c) pb_cv[c][ps] = a.cv[c].bias[ps * CT + (wc * WCB) * 32 + lane];
      if constexpr (S2) {
        pb_t[ps] = a.s2_bias[ps * CT + (wc * WCB) * 32 + lane];
        pb_sc[ps] = a.s2_bias_sc[ps * CT + (wc * WCB) * 32 + lane];
      }
    }
  }
  const int pb_lane = 16 * h;  // byte address of lane 4 * h for ds_bpermute
  auto bias_rows = [&](float v, int i, float4v(&out)[4]) {  // out[q][e] = bias of accumulator row 8 * q + 4 * h + e of cout block i
    int base = pb_lane;
    asm volatile("" : "+v"(v), "+v"(base));  // (or the 16 results / lane addresses, tile-invariant, are hoisted out of the tile loop and stay live)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        out[q][e] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(base + (i * 32 + 8 * q + e) * 4, __builtin_bit_cast(int, v)));
  };
  uint4v keep[NPASS][WCB][WPB][2];  // residual tile saved by an earlier conv of the chain (packed fp16, pair16 layout)
  uint4v hold0[WCB][WPB][2];        // S2, two cout passes: pass 0's t tile while pass 1 still reads the input patches
#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
    for (int i = 0; i < WCB; ++i)
#pragma unroll
      for (int j = 0; j < WPB; ++j)
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) keep[ps][i][j][qq] = uint4v{0u, 0u, 0u, 0u};

  for (; t < ntiles; t += tstep) {
    // keep the tile loop from turning every tile-invariant address term into a live register (see conv_mfma_kernel)
#pragma unroll
    for (int j = 0; j < WPB; ++j) asm volatile("" : "+v"(pj[j]));
    opaque_pixels();
    const bool has_next = t + tstep < ntiles;
    int opix[WPB], gidx[WPB];  // flattened (n, y, x) of this lane's output pixels, GAP partial-sum rows
    auto out_index = [&]() {
#pragma unroll
      for (int j = 0; j < WPB; ++j) {
        const int nn = (t << SPW_L) + (pj[j] >> (2 * HL));
        const bool ok = nn < a.n;
        opix[j] = ok ? nn * HW + (pj[j] & (HW - 1)) : -1;
        gidx[j] = ok ? nn * a.gap_slots + ((mj[j] & (HW - 1)) >> 5) : -1;
      }
    };
    // whole-stage variant: only the last epilogue needs them -- computed there from opaque copies, or the store addresses derived
    // from them are formed up here and live (= spilled) across the whole tile
    if constexpr (!S2 && KEEP) out_index();
    auto out_index_late = [&]() {
#pragma unroll
      for (int j = 0; j < WPB; ++j) asm volatile("" : "+v"(pj[j]), "+v"(mj[j]));
      opaque_pixels();
      out_index();
    };

    if constexpr (LO8) {
      // The tile's input arrived by LDS-DMA as fp16: its e4m3 image is made here, once (every later activation gets its image from the
      // epilogue that writes it).  All regions have landed (patch waves waited before the previous tile's last barrier / in the prologue).
      if (patch_wave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_barrier" ::: "memory");
      for (int it = tid; it < ACT / 16; it += 64 * NW) {
        const int c = it / (REGION / 16), r = it - c * (REGION / 16), q = r / SLOTS, pos = r & (SLOTS - 1);
        const int sl = pos ^ swz(q);                     // channel slot (8 channels) this 16-byte item holds
        const half8 v = *(const half8 *)(smem + (size_t)it * 16);
        uint32_t d0, d1;
        cvt_frag_fp8(v, d0, d1);
        typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
        *(uint2v *)(smem + A8BASE + c * REGION8 + q * KC + ((((sl >> 1) ^ ((q >> 2) & 3)) << 4) | ((sl & 1) << 3))) = uint2v{d0, d1};
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if constexpr (!S2 && NCHUNK == 1) {  // single-region buffer: the next sample's input was requested only after the previous tile's last step
      if (patch_wave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      PHC_MARK(1);
      asm volatile("s_barrier" ::: "memory");
      PHC_MARK(0);
    }
    if constexpr (S2) {
      // ================= stride-2 conv + projection shortcut of the stage, on this tile =================
      // patches 0 and 1 and the first weight step of this tile (issued a tile ago / in the prologue; every wave has a share)
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      PHC_MARK(0);
      int bS[WPB];  // patch pixel of tap (0, 0) for this lane's output pixels
#pragma unroll
      for (int j = 0; j < WPB; ++j) bS[j] = ((pj[j] >> (2 * HL)) * PRS + 2 * ((pj[j] >> HL) & (H - 1))) * PCW + (pj[j] & (H - 1));
      auto put_t = [&](int pass, int i, int j, int qq, uint4v w) {  // this lane: channels cb .. cb+7 of pixel pj[j] -> activation buffer
        const int cb = pass * CT + (wc * WCB + i) * 32 + 16 * qq + 8 * h;
        *(uint4v *)(smem + (cb / KC) * REGION + pj[j] * (KC * 2) + ((((cb % KC) / 8) ^ swz(pj[j])) << 4)) = w;
      };
      if constexpr (WIDE) {
        // both cout passes at once: 8 accumulators; step si = 2 * chunk + hf carries taps [TH * hf, TH * hf + TH) of the chunk for both passes
        float16v acc[NPASS][WCB][WPB], accs[NPASS][WCB][WPB];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
          for (int i = 0; i < WCB; ++i)
#pragma unroll
            for (int j = 0; j < WPB; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) { acc[ps][i][j][r] = 0.f; accs[ps][i][j][r] = 0.f; }
#pragma unroll 1
        for (int chunk = 0; chunk < NCS; ++chunk) {
          const uint32_t pb = lds0 + pbuf(chunk) * PBYTES;
          static_for<2>([&](auto hc) {
            constexpr int hf = decltype(hc)::value;
            if constexpr (hf == 0) {
              if (chunk >= 1 && chunk + PLA < NCS) patch_dma(t, chunk + PLA);  // into the buffer chunk - 1 has finished with
            }
            issue_ring();
            {
              const uint32_t wb = lds0 + (hf ? SOFF1 : SOFF0) + (wc * WCB) * 1024 + lane16;
              half8 fa[2][NPASS][WCB], fb[2][WPB];
              auto issue = [&](auto ic) {
                constexpr int tl = decltype(ic)::value, sl = tl & 1, tt = TH * hf + tl;
                constexpr int te = tt == 9 ? 4 : tt, dy = te / 3, dx = te % 3;  // the 1x1 stride-2 shortcut reads the centre tap's pixel
                constexpr int off = dy * PCW + (dx == 1 ? H + 1 : dx / 2);
                static_for<NPASS * WCB>([&](auto ii) {
                  constexpr int ps = decltype(ii)::value / WCB, i = decltype(ii)::value % WCB;
                  lds_read128<ps * WHALF_S + (tl * CBT + i) * 1024>(fa[sl][ps][i], wb);
                });
                static_for<WPB>([&](auto jj) {
                  constexpr int j = decltype(jj)::value;
                  const int qS = bS[j] + off;
                  lds_read128<0>(fb[sl][j], pb + qS * (KCS * 2) + ((h ^ ((qS >> 3) & 1)) << 4));
                });
              };
              issue(std::integral_constant<int, 0>{});
              static_for<TH>([&](auto ic) {
                constexpr int tl = decltype(ic)::value, sl = tl & 1, tt = TH * hf + tl;
                if constexpr (tl + 1 < TH) issue(std::integral_constant<int, tl + 1>{});
                lds_wait<(tl + 1 < TH ? NPASS * WCB + WPB : 0)>();
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
                  for (int i = 0; i < WCB; ++i) lds_touch(fa[sl][ps][i]);
#pragma unroll
                for (int j = 0; j < WPB; ++j) lds_touch(fb[sl][j]);
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
                  for (int i = 0; i < WCB; ++i)
#pragma unroll
                    for (int j = 0; j < WPB; ++j) {
                      if constexpr (tt == 9) accs[ps][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sl][ps][i], fb[sl][j], accs[ps][i][j], 0, 0, 0);
                      else acc[ps][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sl][ps][i], fb[sl][j], acc[ps][i][j], 0, 0, 0);
                    }
              });
            }
            PHC_MARK(1);
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");  // next weight step and (first half of a chunk) the patch requested above landed
            PHC_MARK(2);
            --ahead;
          });
        }
        // every wave is past the last step's barrier: t = relu(bn1(conv)) -> activation buffer, sc = bn(shortcut) -> residual registers of conv 0
        static_for<NPASS>([&](auto kp) {
          constexpr int ps = decltype(kp)::value;
#pragma unroll
          for (int i = 0; i < WCB; ++i) {
            float4v b1[4], bs[4];
            bias_rows(pb_t[ps], i, b1);
            bias_rows(pb_sc[ps], i, bs);
#pragma unroll
            for (int j = 0; j < WPB; ++j)
              static_for<2>([&](auto qc) {
                constexpr int qq = decltype(qc)::value;
                half4 ht[2], hc[2];
                const half4 none{};
                ht[0] = act_quad<2 * qq>(acc[ps][i][j], a.s2_scale, b1[2 * qq], false, none, true);
                ht[1] = act_quad<2 * qq + 1>(acc[ps][i][j], a.s2_scale, b1[2 * qq + 1], false, none, true);
                hc[0] = act_quad<2 * qq>(accs[ps][i][j], a.s2_scale, bs[2 * qq], false, none, false);
                hc[1] = act_quad<2 * qq + 1>(accs[ps][i][j], a.s2_scale, bs[2 * qq + 1], false, none, false);
                keep[ps][i][j][qq] = pair16(hc[0], hc[1]);
                put_t(ps, i, j, qq, pair16(ht[0], ht[1]));
              });
          }
        });
      } else
      static_for<NPASS>([&](auto kp) {
        constexpr int ps = decltype(kp)::value;
        float16v acc[WCB][WPB], accs[WCB][WPB];
#pragma unroll
        for (int i = 0; i < WCB; ++i)
#pragma unroll
          for (int j = 0; j < WPB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; accs[i][j][r] = 0.f; }
#pragma unroll 1
        for (int chunk = 0; chunk < NCS; ++chunk) {
          const int si = ps * NCS + chunk;  // stride-2 step index in this tile
          if (si >= 1 && si + PLA < NS) patch_dma(t, si + PLA);  // (HBM: first) into the buffer step si - 1 has finished with
          issue_ring();
          {
            const uint32_t wb = lds0 + ((si & 1) ? SOFF1 : SOFF0) + (wc * WCB) * 1024 + lane16;
            const uint32_t pb = lds0 + pbuf(si) * PBYTES;
            half8 fa[2][WCB], fb[2][WPB];
            auto issue = [&](auto ic) {
              constexpr int tt = decltype(ic)::value, sl = tt & 1;
              constexpr int te = tt == 9 ? 4 : tt, dy = te / 3, dx = te % 3;  // the 1x1 stride-2 shortcut reads the centre tap's pixel
              constexpr int off = dy * PCW + (dx == 1 ? H + 1 : dx / 2);
              static_for<WCB>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                lds_read128<(tt * CBT + i) * 1024>(fa[sl][i], wb);
              });
              static_for<WPB>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                const int qS = bS[j] + off;
                lds_read128<0>(fb[sl][j], pb + qS * (KCS * 2) + ((h ^ ((qS >> 3) & 1)) << 4));
              });
            };
            issue(std::integral_constant<int, 0>{});
            static_for<TAPS_S>([&](auto ic) {
              constexpr int tt = decltype(ic)::value, sl = tt & 1;
              if constexpr (tt + 1 < TAPS_S) issue(std::integral_constant<int, tt + 1>{});
              lds_wait<(tt + 1 < TAPS_S ? WCB + WPB : 0)>();
#pragma unroll
              for (int i = 0; i < WCB; ++i) lds_touch(fa[sl][i]);
#pragma unroll
              for (int j = 0; j < WPB; ++j) lds_touch(fb[sl][j]);
#pragma unroll
              for (int i = 0; i < WCB; ++i)
#pragma unroll
                for (int j = 0; j < WPB; ++j) {
                  if constexpr (tt == 9) accs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sl][i], fb[sl][j], accs[i][j], 0, 0, 0);
                  else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sl][i], fb[sl][j], acc[i][j], 0, 0, 0);
                }
            });
          }
          PHC_MARK(1);
          asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");  // next weight step (ring waves) and next patch (patch waves) landed
          PHC_MARK(2);
          --ahead;
        }
        // t = relu(bn1(conv)) -> activation buffer (pass 0 of 2: held until pass 1 has read its patches -- they overlap the buffer);
        // sc = bn(shortcut) -> residual registers of conv 0
#pragma unroll
        for (int i = 0; i < WCB; ++i) {
          float4v b1[4], bs[4];
          if constexpr (PBIAS) {
            bias_rows(pb_t[ps], i, b1);
            bias_rows(pb_sc[ps], i, bs);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              b1[q] = *(const float4v *)(a.s2_bias + ps * CT + (wc * WCB + i) * 32 + 4 * h + 8 * q);
              bs[q] = *(const float4v *)(a.s2_bias_sc + ps * CT + (wc * WCB + i) * 32 + 4 * h + 8 * q);
            }
          }
#pragma unroll
          for (int j = 0; j < WPB; ++j)
            static_for<2>([&](auto qc) {
              constexpr int qq = decltype(qc)::value;
              half4 ht[2], hc[2];
              const half4 none{};
              ht[0] = act_quad<2 * qq>(acc[i][j], a.s2_scale, b1[2 * qq], false, none, true);
              ht[1] = act_quad<2 * qq + 1>(acc[i][j], a.s2_scale, b1[2 * qq + 1], false, none, true);
              hc[0] = act_quad<2 * qq>(accs[i][j], a.s2_scale, bs[2 * qq], false, none, false);
              hc[1] = act_quad<2 * qq + 1>(accs[i][j], a.s2_scale, bs[2 * qq + 1], false, none, false);
              keep[ps][i][j][qq] = pair16(hc[0], hc[1]);
              const uint4v wt = pair16(ht[0], ht[1]);
              if constexpr (NPASS == 2 && ps == 0) hold0[i][j][qq] = wt;  // pass 1 still reads the patches, which overlap the buffer
              else put_t(ps, i, j, qq, wt);
            });
        }
        if constexpr (NPASS == 2 && ps == 1) {
#pragma unroll
          for (int i = 0; i < WCB; ++i)
#pragma unroll
            for (int j = 0; j < WPB; ++j)
#pragma unroll
              for (int qq = 0; qq < 2; ++qq) put_t(0, i, j, qq, hold0[i][j][qq]);
        }
      });
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      PHC_MARK(3);
    }

    static_for<NCONV>([&](auto kc) {
      constexpr int cvi = decltype(kc)::value;
      constexpr bool lastc = cvi == NCONV - 1;
      const ChainConv &cv = a.cv[cvi];
      // the chain (host: run_chain3): conv2(+sc from HBM, saved) -> conv1 -> conv2(+saved tile); every conv is followed by a ReLU
      // (S2: conv 0's residual sc is not in HBM but in the registers the stride-2 phase left it in)
      // (KEEP = false: b0 goes through HBM instead of the registers: conv 0 stores it, the last conv loads it as cv.res)
      constexpr int RES = cvi == 0 ? (S2 ? 2 : 1) : cvi == 2 ? (KEEP ? 2 : 1) : 0;
      constexpr bool SAVE = KEEP && cvi == 0;
      constexpr bool RES_LATE = !KEEP;  // residual loads after the last step's MFMA loop (the fragment registers are free then)
      uint4v hold[WCB][WPB][2];  // NPASS == 2: pass 0's activated tile until pass 1 has finished reading the buffer
      // epilogue of the stage's last conv for cout pass kp: + bias + residual, ReLU -> HBM and / or GAP sums
      auto std_epi = [&](auto kp, float16v(&acc)[WCB][WPB], uint4v(&resv)[WCB][WPB][2]) {
        constexpr int ps = decltype(kp)::value;
        float4v bq[WCB][4], bsq[1][4];
#pragma unroll
        for (int i = 0; i < WCB; ++i) {
          if constexpr (PBIAS) bias_rows(pb_cv[cvi][ps], i, bq[i]);
          else {
#pragma unroll
            for (int q = 0; q < 4; ++q) bq[i][q] = *(const float4v *)(cv.bias + ps * CT + (wc * WCB + i) * 32 + 4 * h + 8 * q);
          }
        }
        ConvArgs ea{};
        ea.y = a.y; ea.gap = a.gap; ea.gap_slots = a.gap_slots; ea.gap_l = a.gap_l; ea.acc_scale = cv.acc_scale; ea.relu = 1;
        ea.y_c16 = a.y_c16; ea.hout_l = HL;
        ea.res = RES ? (const void *)a.x : nullptr;  // non-NULL = "add resv"
        float16v acc_sc[1][1];
        uint4v resl[1][1][2];
        if constexpr (RES == 2) {
#pragma unroll
          for (int i = 0; i < WCB; ++i)
#pragma unroll
            for (int j = 0; j < WPB; ++j)
#pragma unroll
              for (int qq = 0; qq < 2; ++qq) resv[i][j][qq] = keep[ps][i][j][qq];
        }
        int he = h, pe = p;
        asm volatile("" : "+v"(he), "+v"(pe));  // nothing of the epilogue's lane arithmetic is hoisted out of the tile loop
        conv_epilogue<C, CT, WCB, WPB, false, 1>(ea, ps, wc, he, pe, opix, gidx, acc, acc_sc, bq, bsq, resv, resl);
      };
      if constexpr (WIDE) {
        // both cout passes at once: 4 accumulators.  A step is items [WI * s, WI * s + WI) of the chunk's 36 (tap, k16) items; the pair of steps
        // (2g, 2g + 1) covers taps 3g .. 3g + 2 and is unrolled statically (item = position in the pair, hf = which step of the pair)
        float16v acc[NPASS][WCB][WPB];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
          for (int i = 0; i < WCB; ++i)
#pragma unroll
            for (int j = 0; j < WPB; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r) acc[ps][i][j][r] = 0.f;
#pragma unroll 1
        for (int chunk = 0; chunk < NCHUNK; ++chunk) {
          const uint32_t pl = lds0 + chunk * REGION;
#pragma unroll 1
          for (int g = 0; g < NG; ++g) {
            static_for<2>([&](auto hc) {
              constexpr int hf = decltype(hc)::value;
              issue_ring();  // the step after this one, into the slot read one step ago
              {
                const uint32_t wb = lds0 + ACT + slot_rd * WCHUNK + (wc * WCB) * 1024 + lane16;
                half8 fa[2][NPASS][WCB], fb[2][WPB];
                uint32_t rowa[WPB], hs[WPB];
                auto issue = [&](auto ic) {
                  constexpr int item = decltype(ic)::value, il = item - WI * hf, sl = item & 1, tt = item / KS, ks = item % KS;
                  if constexpr (ks == 0 || il == 0) {  // a tap begins, or the step begins inside one
                    const int tp = g * GT + tt, dy = tp / 3, dx = tp - dy * 3;
#pragma unroll
                    for (int j = 0; j < WPB; ++j) {
                      const int yy = ((pj[j] >> HL) & (H - 1)) + dy - 1, xx = (pj[j] & (H - 1)) + dx - 1;
                      const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)H;  // else: conv padding
                      const int q = ok ? pj[j] + (dy - 1) * H + (dx - 1) : pj[j];
                      rowa[j] = ok ? pl + q * (KC * 2) : 0x100000u;  // beyond the LDS: the read returns zeros
                      hs[j] = (h * 16) ^ (swz(q) << 4);
                    }
                  }
                  static_for<NPASS * WCB>([&](auto ii) {
                    constexpr int ps = decltype(ii)::value / WCB, i = decltype(ii)::value % WCB;
                    lds_read128<ps * WHALF + (il * CBT + i) * 1024>(fa[sl][ps][i], wb);
                  });
                  static_for<WPB>([&](auto jj) { lds_read128<0>(fb[sl][decltype(jj)::value], rowa[decltype(jj)::value] + (hs[decltype(jj)::value] ^ (ks * 32))); });
                };
                issue(std::integral_constant<int, WI * hf>{});
                static_for<WI>([&](auto ic) {
                  constexpr int il = decltype(ic)::value, item = WI * hf + il, sl = item & 1;
                  if constexpr (il + 1 < WI) issue(std::integral_constant<int, item + 1>{});
                  lds_wait<(il + 1 < WI ? NPASS * WCB + WPB : 0)>();
#pragma unroll
                  for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
                    for (int i = 0; i < WCB; ++i) lds_touch(fa[sl][ps][i]);
#pragma unroll
                  for (int j = 0; j < WPB; ++j) lds_touch(fb[sl][j]);
#pragma unroll
                  for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
                    for (int i = 0; i < WCB; ++i)
#pragma unroll
                      for (int j = 0; j < WPB; ++j) acc[ps][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sl][ps][i], fb[sl][j], acc[ps][i][j], 0, 0, 0);
                });
              }
              PHC_MARK(4 + 3 * cvi);
              if (ring_wave) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next ring step has landed
              asm volatile("s_barrier" ::: "memory");
              PHC_MARK(5 + 3 * cvi);
              --ahead;
              slot_rd ^= 1;
            });
          }
        }
        // every wave is past the last step's barrier: nobody reads the activation buffer any more
        if constexpr (lastc) {
          if (has_next) {  // all patch buffers of the next tile
#pragma unroll
            for (int i = 0; i < NPB; ++i) patch_dma(t + tstep, i);
          }
          out_index_late();
          static_for<NPASS>([&](auto kp) {
            uint4v resv[WCB][WPB][2];
            std_epi(kp, acc[decltype(kp)::value], resv);
          });
          PHC_MARK(6 + 3 * cvi);
        } else {
          // + bias (+ residual) (ReLU) -> fp16 -> back into the activation buffer (input of the next conv), both passes
          static_for<NPASS>([&](auto kp) {
            constexpr int ps = decltype(kp)::value;
#pragma unroll
            for (int i = 0; i < WCB; ++i) {
              float4v bi[4];
              bias_rows(pb_cv[cvi][ps], i, bi);
#pragma unroll
              for (int j = 0; j < WPB; ++j)
                static_for<2>([&](auto qc) {
                  constexpr int qq = decltype(qc)::value;
                  half4 ra{}, rb{}, hq[2];
                  if constexpr (RES != 0) unpair16(keep[ps][i][j][qq], ra, rb);
                  hq[0] = act_quad<2 * qq>(acc[ps][i][j], cv.acc_scale, bi[2 * qq], RES != 0, ra, true);
                  hq[1] = act_quad<2 * qq + 1>(acc[ps][i][j], cv.acc_scale, bi[2 * qq + 1], RES != 0, rb, true);
                  const uint4v w = pair16(hq[0], hq[1]);
                  if constexpr (SAVE) keep[ps][i][j][qq] = w;
                  const int cb = ps * CT + (wc * WCB + i) * 32 + 16 * qq + 8 * h;  // this lane: channels cb .. cb+7 of pixel pj[j]
                  *(uint4v *)(smem + (cb / KC) * REGION + pj[j] * (KC * 2) + ((((cb % KC) / 8) ^ swz(pj[j])) << 4)) = w;
                });
            }
          });
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          PHC_MARK(6 + 3 * cvi);
        }
      } else
      static_for<NPASS>([&](auto kp) {
        constexpr int ps = decltype(kp)::value;
        constexpr bool last = lastc && ps == NPASS - 1;  // the very last K loop over the buffer for this sample
        float16v acc[WCB][WPB];
#pragma unroll
        for (int i = 0; i < WCB; ++i)
#pragma unroll
          for (int j = 0; j < WPB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        uint4v resv[WCB][WPB][2];

#pragma unroll 1
        for (int chunk = 0; chunk < NCHUNK; ++chunk) {
          const uint32_t pl = lds0 + chunk * REGION;
          auto do_step = [&](int g, auto nitem_c) {
            issue_ring();  // step PFD ahead of the one computed now (into the slot read in step g-1)
            // the last K loop has finished reading region chunk-1: the next sample's input may land there
            if (!S2 && last && has_next && g == 0 && chunk >= 1) dma_region(t + tstep, chunk - 1);
            if (RES == 1 && !RES_LATE && chunk == NCHUNK - 1 && g == NG - 1) {  // HBM residual: flies under the last weight step
#pragma unroll
              for (int i = 0; i < WCB; ++i)
#pragma unroll
                for (int j = 0; j < WPB; ++j) {
                  const size_t o = (size_t)(opix[j] >= 0 ? opix[j] : 0) * C + ps * CT + (wc * WCB + i) * 32 + 8 * h;
#pragma unroll
                  for (int qq = 0; qq < 2; ++qq) resv[i][j][qq] = *(const uint4v *)((const _Float16 *)cv.res + o + 16 * qq);
                }
            }
            {
              constexpr int NITEM = decltype(nitem_c)::value, NR = WP * WCB + WPB;
              const uint32_t wb = lds0 + ACT + slot_rd * WCHUNK + (wc * WCB) * 1024 + lane16;
              const uint32_t wb8 = lds0 + ACT + slot_rd * WCHUNK + WP * WPLANE + (wc * WCB) * 2048 + lane16;  // LO8: the FP8 fragments of this wave's cout blocks
              half8 fa[FD + 1][WP][WCB], fb[FD + 1][WPB];
              half8 f8[LO8 ? WCB : 1][2];   // LO8: the tap's FP8 A fragments (32 bytes per lane), requested with the tap's second item
              half8 g8[LO8 ? WPB : 1][2];   // ... and its B fragments (channels 32 h .. 32 h + 31 of the lane's pixel from the e4m3 image), with the third
              uint32_t rowa8[LO8 ? WPB : 1], sw8[LO8 ? WPB : 1];
              int lo8_sa = 0;
              if constexpr (LO8) lo8_sa = cv.lo8_scale;
              uint32_t rowa[WPB], hs[WPB], mcur[WPB], mvs[FD + 1][WPB];
              auto issue = [&](auto ic) {
                constexpr int item = decltype(ic)::value, sl = item % (FD + 1), tt = item / KS, ks = item % KS;
                if constexpr (ks == 0) {
                  const int tp = g * GT + tt, dy = tp / 3, dx = tp - dy * 3;
#pragma unroll
                  for (int j = 0; j < WPB; ++j) {
                    const int yy = ((pj[j] >> HL) & (H - 1)) + dy - 1, xx = (pj[j] & (H - 1)) + dx - 1;
                    const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)H;  // else: conv padding
                    const int q = ok ? pj[j] + (dy - 1) * H + (dx - 1) : pj[j];
                    rowa[j] = pl + q * (KC * 2);
                    if constexpr (OOBZ) {
                      if (!ok) rowa[j] = 0x100000u;  // beyond the LDS: the read returns zeros, no mask needed
                    }
                    hs[j] = (h * 16) ^ (swz(q) << 4);
                    mcur[j] = ok ? 0xFFFFFFFFu : 0u;
                    if constexpr (LO8) {
                      rowa8[j] = ok ? lds0 + A8BASE + chunk * REGION8 + q * KC : 0x100000u;  // (padding taps: zeros from beyond the LDS, as above)
                      sw8[j] = (uint32_t)((q >> 2) & 3);
                    }
                  }
                }
#pragma unroll
                for (int j = 0; j < WPB; ++j) mvs[sl][j] = mcur[j];
                static_for<WP * WCB>([&](auto ii) {
                  constexpr int sp = decltype(ii)::value / WCB, i = decltype(ii)::value % WCB;
                  lds_read128<sp * WPLANE + ((tt * KS + ks) * CBT + i) * 1024>(fa[sl][sp][i], wb);
                });
                static_for<WPB>([&](auto jj) { lds_read128<0>(fb[sl][decltype(jj)::value], rowa[decltype(jj)::value] + (hs[decltype(jj)::value] ^ (ks * 32))); });
                if constexpr (LO8 && ks == 1) {  // (with the tap's SECOND item: the previous tap's lo MFMAs, issued at its last item, have read f8 by then)
                  static_for<WCB>([&](auto ii) {
                    constexpr int i = decltype(ii)::value;
                    lds_read128<(tt * CBT + i) * 2048>(f8[i][0], wb8);
                    lds_read128<(tt * CBT + i) * 2048 + 1024>(f8[i][1], wb8);
                  });
                }
                if constexpr (LO8 && ks == 2) {  // the e4m3 activation fragments of the tap: 16-channel slots 2h and 2h + 1 of the lane's pixel
                  static_for<WPB>([&](auto jj) {
                    constexpr int j = decltype(jj)::value;
                    lds_read128<0>(g8[j][0], rowa8[j] + (((2 * h) ^ sw8[j]) << 4));
                    lds_read128<0>(g8[j][1], rowa8[j] + (((2 * h + 1) ^ sw8[j]) << 4));
                  });
                }
              };
              issue(std::integral_constant<int, 0>{});
              if constexpr (NITEM > 1 && FD > 1) issue(std::integral_constant<int, 1>{});
              if constexpr (NITEM > 2 && FD > 2) issue(std::integral_constant<int, 2>{});
              static_for<NITEM>([&](auto ic) {
                constexpr int item = decltype(ic)::value, sl = item % (FD + 1);
                if constexpr (item + FD < NITEM) issue(std::integral_constant<int, item + FD>{});
                // reads younger than this item's: those of the next FD items (LO8: + the FP8 fragments that ride on a tap's second item)
                constexpr int younger = (NITEM - 1 - item < FD ? NITEM - 1 - item : FD) * NR + ((LO8 && item + 1 < NITEM && (item + 1) % KS == 1) ? 2 * WCB : 0) +
                                        ((LO8 && item + 1 < NITEM && (item + 1) % KS == 2) ? 2 * WPB : 0);
                lds_wait<younger>();
#pragma unroll
                for (int sp = 0; sp < WP; ++sp)
#pragma unroll
                  for (int i = 0; i < WCB; ++i) lds_touch(fa[sl][sp][i]);
                half8 bm[WPB];
#pragma unroll
                for (int j = 0; j < WPB; ++j) {
                  lds_touch(fb[sl][j]);
                  bm[j] = fb[sl][j];
                  if constexpr (!OOBZ) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) ((uint32_t *)&bm[j])[e] &= mvs[sl][j];
                  }
                }
                // (W2: all hi products of the item, then all lo products -- per accumulator hi then lo, and no MFMA depends on its predecessor)
#pragma unroll
                for (int sp = 0; sp < WP; ++sp)
#pragma unroll
                  for (int i = 0; i < WCB; ++i)
#pragma unroll
                    for (int j = 0; j < WPB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sl][sp][i], bm[j], acc[i][j], 0, 0, 0);
                if constexpr (LO8) {
                  if constexpr (item % KS == KS - 1) {  // the tap's lo product: one FP8 MFMA per accumulator over all 64 channels of the chunk
#pragma unroll
                    for (int i = 0; i < WCB; ++i) { lds_touch(f8[i][0]); lds_touch(f8[i][1]); }
#pragma unroll
                    for (int j = 0; j < WPB; ++j) { lds_touch(g8[j][0]); lds_touch(g8[j][1]); }
#pragma unroll
                    for (int i = 0; i < WCB; ++i)
#pragma unroll
                      for (int j = 0; j < WPB; ++j) acc[i][j] = mfma_lo8(f8[i][0], f8[i][1], g8[j][0], g8[j][1], acc[i][j], lo8_sa);
                  }
                }
              });
            }
            if constexpr (RES == 1 && RES_LATE) {
              // (defined in every iteration by the empty asm: not live across any step's MFMA loop, only from here to the epilogue)
#pragma unroll
              for (int i = 0; i < WCB; ++i)
#pragma unroll
                for (int j = 0; j < WPB; ++j)
#pragma unroll
                  for (int qq = 0; qq < 2; ++qq) asm volatile("" : "=v"(resv[i][j][qq]));
              if (chunk == NCHUNK - 1 && g == NG - 1) {
                out_index_late();
                const _Float16 *resb = (const _Float16 *)KARG(const void *, cv[cvi].res);
                const bool res0_c16 = cvi == 0 && KARG(int, res0_c16) != 0;
#pragma unroll
                for (int i = 0; i < WCB; ++i)
#pragma unroll
                  for (int j = 0; j < WPB; ++j) {
                    // cvi == 0: sc, written NHWC by the stride-2 kernel; else b0, written by this wave below in its own order
                    // (lane-linear 1 KiB blocks: a quad of lanes touches ONE 64-byte span instead of four cache lines)
                    const int op0 = opix[j] >= 0 ? opix[j] : 0;
                    const size_t o = cvi != 0       ? (((size_t)t * NW + wave) * (WCB * WPB * 2) + (i * WPB + j) * 2) * 512 + lane * 8
                                     : res0_c16 ? ((((size_t)(op0 >> (2 * HL)) * (C / 16) + ((ps * CT + (wc * WCB + i) * 32) >> 4)) << (2 * HL)) + (op0 & (HW - 1))) * 16 + 8 * h
                                                : (size_t)op0 * C + ps * CT + (wc * WCB + i) * 32 + 8 * h;
                    // (asm loads: the compiler does not track them, so the epilogue's first use is not preceded by its
                    // s_waitcnt vmcnt(0) -- which would also drain the next sample's input DMA issued in between; the wait is below)
#pragma unroll
                    for (int qq = 0; qq < 2; ++qq) {
                      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(resv[i][j][qq]) : "v"(resb + o + (cvi != 0 ? 512 : res0_c16 ? HW * 16 : 16) * qq) : "memory");
                    }
                  }
              }
            }
            // ---- end of step: next ring step landed (ring waves); next sample's regions landed (patch waves) where the
            // following step reads them ----
            PHC_MARK(4 + 3 * cvi);
            if constexpr (SPLIT_ROLES) {
              if (ring_wave) {  // the step after this one has landed; the ahead - 2 younger ones may still fly
                if (PFD >= 3 && ahead >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPWR) : "memory");
                else if (PFD >= 2 && ahead >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPWR) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              } else {
                const bool before_next_sample = NCHUNK > 1 && last && chunk == NCHUNK - 1 && g == NG - 1;   // regions 0 .. NCHUNK-2
                const bool before_last_region = cvi == 0 && ps == 0 && chunk == NCHUNK - 2 && g == NG - 1;  // region NCHUNK-1
                if (before_next_sample || before_last_region) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              }
            } else {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if constexpr (RES == 1 && RES_LATE) {  // the residual tile requested above (every wave)
              if (chunk == NCHUNK - 1 && g == NG - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("s_barrier" ::: "memory");
            PHC_MARK(5 + 3 * cvi);
            --ahead;
            if (++slot_rd == NBUF) slot_rd = 0;
          };
          // (a shorter last tap group is peeled: both item counts inside one loop body, selected by a branch, cost 900 B of scratch)
#pragma unroll 1
          for (int g = 0; g < (GT_LAST != GT ? NG - 1 : NG); ++g) do_step(g, std::integral_constant<int, GT * KS>{});
          if constexpr (GT_LAST != GT) do_step(NG - 1, std::integral_constant<int, GT_LAST * KS>{});
        }
        // every wave is past the last step's barrier
        if constexpr (lastc) {
          if constexpr (last) {  // nobody reads the activation buffer any more
            if constexpr (S2) {
              if (has_next) {  // all patch buffers of the next tile
#pragma unroll
                for (int i = 0; i < NPB; ++i) patch_dma(t + tstep, i);
              }
            } else if (has_next) dma_region(t + tstep, NCHUNK - 1);
          }
          if constexpr (S2 || !KEEP) out_index_late();
          // !KEEP (8 accumulators + the residual tile in registers): the same epilogue one 32-cout block at a time, so that only one
          // block's 16 bias values are live (both blocks' at once, as above, spilled)
          auto blk_epi = [&]() {
            ConvArgs ea{};
            ea.y = KARG(void *, y); ea.gap = KARG(float *, gap); ea.gap_slots = KARG(int, gap_slots); ea.gap_l = KARG(int, gap_l);
            ea.acc_scale = KARG(float, cv[cvi].acc_scale); ea.relu = 1;
            ea.y_c16 = KARG(int, y_c16); ea.hout_l = HL;
            ea.res = RES ? (const void *)ea.y : nullptr;  // (only its non-NULLness is looked at)
            float16v acc_sc[1][1];
            uint4v resl[1][1][2];
            float4v bsq[1][4];
#pragma unroll
            for (int i = 0; i < WCB; ++i) {
              float4v bq1[1][4];
              bias_rows(pb_cv[cvi][ps], i, bq1[0]);
              if (i) out_index_late();  // (recomputed per block: two 64-bit GAP row offsets kept across block 0 were spilled)
              int he = h, pe = p;
              asm volatile("" : "+v"(he), "+v"(pe));
              conv_epilogue<C, CT, 1, WPB, false, 1>(ea, ps, wc * WCB + i, he, pe, opix, gidx, reinterpret_cast<float16v(&)[1][WPB]>(acc[i]), acc_sc, bq1, bsq,
                                                     reinterpret_cast<const uint4v(&)[1][WPB][2]>(resv[i]), resl);
            }
          };
          if constexpr (!KEEP && PBIAS) blk_epi();
          else std_epi(kp, acc, resv);
          PHC_MARK(6 + 3 * cvi);
        } else {
          // + bias (+ residual) (ReLU) -> fp16 -> back into the activation buffer (input of the next conv)
          _Float16 *yb0 = nullptr;  // !KEEP: HBM copy of this conv's output (the later residual), private layout (see the loads)
          if constexpr (!KEEP) yb0 = (_Float16 *)KARG(void *, cv[cvi].y);
          // (lane half from a rematerialised lane id: h itself, kept live over the step loops, was spilled in the 64-channel chain and
          // its reload's s_waitcnt vmcnt(0) drained the weight ring prefetch)
          const int hm = KEEP ? h : (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) >> 5;
          auto put = [&](int pass, int i, int j, int qq, uint4v w) {  // this lane: channels cb .. cb+7 of pixel pj[j]
            const int cb = pass * CT + (wc * WCB + i) * 32 + 16 * qq + 8 * hm;
            *(uint4v *)(smem + (cb / KC) * REGION + pj[j] * (KC * 2) + ((((cb % KC) / 8) ^ swz(pj[j])) << 4)) = w;
            if constexpr (LO8) {  // ... and their e4m3 image: 16-channel slot (cb % KC) / 16 swizzled with the pixel index, 8 bytes at (cb % 16)
              uint32_t d0, d1;
              cvt_frag_fp8(*(const half8 *)&w, d0, d1);
              typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
              *(uint2v *)(smem + A8BASE + (cb / KC) * REGION8 + pj[j] * KC + (((((cb % KC) >> 4) ^ ((pj[j] >> 2) & 3)) << 4) | (cb & 8))) = uint2v{d0, d1};
            }
          };
#pragma unroll
          for (int i = 0; i < WCB; ++i) {
            float4v bi[4];
            if constexpr (PBIAS) bias_rows(pb_cv[cvi][ps], i, bi);
            else {
#pragma unroll
              for (int q = 0; q < 4; ++q) bi[q] = *(const float4v *)(cv.bias + ps * CT + (wc * WCB + i) * 32 + 4 * h + 8 * q);
            }
#pragma unroll
            for (int j = 0; j < WPB; ++j)
              static_for<2>([&](auto qc) {
                constexpr int qq = decltype(qc)::value;
                half4 ra{}, rb{}, hq[2];
                if constexpr (RES != 0) unpair16(RES == 2 ? keep[ps][i][j][qq] : resv[i][j][qq], ra, rb);
                hq[0] = act_quad<2 * qq>(acc[i][j], cv.acc_scale, bi[2 * qq], RES != 0, ra, true);
                hq[1] = act_quad<2 * qq + 1>(acc[i][j], cv.acc_scale, bi[2 * qq + 1], RES != 0, rb, true);
                const uint4v w = pair16(hq[0], hq[1]);
                if constexpr (SAVE) keep[ps][i][j][qq] = w;
                if constexpr (!KEEP) {  // the later residual goes through HBM
                  if (yb0) *(uint4v *)(yb0 + (((size_t)t * NW + wave) * (WCB * WPB * 2) + (i * WPB + j) * 2 + qq) * 512 + lane * 8) = w;
                }
                if constexpr (ps == NPASS - 1) put(ps, i, j, qq, w);
                else hold[i][j][qq] = w;
              });
          }
          if constexpr (ps == NPASS - 1) {
            if constexpr (NPASS == 2) {
#pragma unroll
              for (int i = 0; i < WCB; ++i)
#pragma unroll
                for (int j = 0; j < WPB; ++j)
#pragma unroll
                  for (int qq = 0; qq < 2; ++qq) put(0, i, j, qq, hold[i][j][qq]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          }
          PHC_MARK(6 + 3 * cvi);
        }
      });
    });
  }
  PHC_FLUSH((C == 256 ? 2 : 0) + (S2 ? 1 : 0));
}

template <int C, int HL, int SPW_L, int WCB, int WPB, int WAVES_C, int WAVES_P, int GT, int RB, int FD, int MINW, int NCONV, bool SPLIT_ROLES, bool S2 = false, bool KEEP = true, bool OOBZ = false, bool W2 = false, bool LO8 = false>
__global__ __launch_bounds__(64 * WAVES_C * WAVES_P, MINW) void chain_kernel(const ChainArgs a) {
  chain_body<C, HL, SPW_L, WCB, WPB, WAVES_C, WAVES_P, GT, RB, FD, MINW, NCONV, SPLIT_ROLES, S2, KEEP, OOBZ, W2, LO8>(a);
}
// The whole 256-channel stage with both cout passes per wave (WIDE above): chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, .., 2, 3, true, true, true, true>'s
// tiling, fragment reads one item ahead.  Padding from beyond the LDS only: devices that fail the LDS probe keep chain_kernel.
__global__ __launch_bounds__(512, 2) void stage256_wide_kernel(const ChainArgs a) {
  chain_body<256, 3, 1, 2, 1, 2, 4, 3, 2, 1, 2, 3, true, true, true, true, false, false, true>(a);
}

