// mlt_layer0_kernel.inc -- layer0_stream_kernel: ALL of layer0 (both BasicBlocks) of a 128 x 128 CU in one launch; part of mlt_kernels.hip.
// ---------------------------------------------------------------------------------------------
// Round 5.  The two-launch form (stem_block_kernel -> b0 in HBM -> block32_kernel) works on 16 x 32 tiles: every tile re-stages a halo
// (1.4x reads of b0, 1.27x recompute of t and of layer0.1's first conv) and b0 -- 256 KiB per CU -- makes a round trip through HBM.  This kernel
// STREAMS the map instead: one workgroup owns a whole CU and walks it top to bottom, whole 64-pixel rows at a time, through four stages
//     S1  t   = relu(bn1(conv1(stem x)))                  composed 5x5 stride-2 conv of the raw planes (+ border k-steps; see stem5_kernel)
//     S2  b0  = relu(bn2(conv2(t)) + bn(shortcut(stem x)))  (arch:52-57 with the projection shortcut, arch:44-50)
//     S3  u   = relu(bn1'(conv1'(b0)))                     layer0.1
//     S4  out = relu(bn2'(conv2'(u)) + b0)                 -> HBM, NHWC fp16
// that hand rows to each other through small LDS rings (8 rows of 66 pixels x 80 B per map: a 3x3 conv needs the rows above and below, nothing
// else), so no pixel of any map is computed or staged twice and only the raw planes (64 KiB) come in and the block output (256 KiB) goes out.
// 16 waves: wave = 4 * stage + unit, unit = (row parity, 32-pixel half of the row).  A step advances every stage by two rows; stage s works on
// rows 2k + parity - 3s (three rows behind its producer: the row below its own must exist), and ONE barrier ends the step.  The four waves of a
// SIMD (wave & 3 = unit) are the four stages of one unit, so every SIMD carries the same MFMA load (5 + 20 + 18 + 18 per step) and a wave in its
// epilogue or waiting for LDS is covered by three others.  The conv weights (18 A fragments) live in each wave's registers for the whole launch;
// per MFMA one activation fragment (ds_read_b128) is read.  The workgroup is persistent over CUs and the pipeline never drains between them:
// rows are numbered through (row g of the workgroup = row g & 63 of its CU g >> 6), padding rows are a shared zero row.
// Arithmetic: the k order, the accumulators and the epilogue expressions are those of stem_block_kernel / block32_kernel -- the results are
// bit-identical to the two-launch form (tests: test_layer0_stream_is_bit_identical).  Fast arithmetic only (single fp16 plane).
// ---------------------------------------------------------------------------------------------
#ifndef CFG_L0_PD
#define CFG_L0_PD 4      // activation fragments in flight per wave (x 4 VGPRs; the waves have 128)
#endif
#ifndef CFG_L0_RD
#define CFG_L0_RD 4      // raw rows in flight per S1 wave (steps between a row's global load and its conversion into LDS)
#endif
#ifndef CFG_L0_PRIO
#define CFG_L0_PRIO 0    // wave priority by stage: 1: S1 highest .. S4 lowest, 2: the reverse (staggers the four waves of a SIMD instead of round-robin MFMA issue)
#endif
#ifndef CFG_L0_XPRE
#define CFG_L0_XPRE 1    // 1: the first fragments of a wave's next row are requested before the barrier that ends the step
#endif
#ifndef CFG_L0_PKEPI
#define CFG_L0_PKEPI 1   // 1: S3 / S4 epilogues in packed arithmetic (act_quad) instead of block32_kernel's scalar expressions (same values)
#endif
#ifndef CFG_L0_KO
#define CFG_L0_KO 0      // measurement only (results are wrong): 1 no activation-fragment reads, 2 no MFMAs in the 3x3 convs, 4 no epilogues, 8 no barrier per step
#endif
#ifndef CFG_L0_MAP
#define CFG_L0_MAP 0     // 0: wave = 4 * stage + unit (a SIMD hosts the four stages of one unit); 1: wave = 4 * unit + stage
#endif
// F5 (second half of round 5): the stride-2 conv that opens layer1 (layer1.0.conv1 + its projection shortcut, 32 -> 64 channels, arch:44-55) joins
// the pipeline as a fifth stage S5 -- conv_mfma_kernel<32, 64, 2, ...>'s arithmetic (tap-major k order, the shortcut as tap 9 in its own accumulator,
// conv_epilogue's expressions), one 32-pixel output row per step and wave, one wave per 32 output channels.  S4 then hands its rows to S5 through a
// fourth ring and layer0's output (256 KiB per CU written, read once more by the stride-2 launch) never exists in HBM; t and sc leave as that
// launch wrote them (t NHWC, sc chunk-major for the 64-channel chain).  The two extra waves come from S1: two waves (one per 32-pixel half) carry
// both row parities -- it has the fewest MFMAs by far -- and fetch two raw rows each with all 64 lanes.  Rings of 6 rows (t, u, out; b0 keeps 8: its
// residual use) make room: 27 map rows = 139 KiB.
// Round 6, M16 = true (the default): the 3x3 conv stages (S2 .. S5) issue v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_32x32x16_f16 -- bit for bit the same
// sums (one 16x16x32 MFMA = two chained 32x32x16 over the same 32 k values: scripts/probes/mfma_shape_bits_probe.hip), a 13 % higher clock under the power cap
// (profiles/r06a_mfma_shape_probe.txt).  Per tap (32 input channels = one k step) a wave runs 2 cout blocks x 2 pixel halves = four MFMAs on two weight
// fragments (16 couts x 32 cin, gathered at load time from the same packed weights) and two activation fragments (16 pixels x 32 cin, ONE ds_read_b128 per
// lane): 18 + 18 fragments per row and 16 accumulator registers as before; a lane ends up with 4 consecutive channels of two pixels per cout block, so the
// epilogues need TWO bias quads instead of four and write 8-byte pieces without permlane pairing.  S1 (five k = 16 steps per row + border steps) keeps the
// 32x32x16 shape: its accumulators never meet another stage's.  M16 = false is round 5's form (MLT_TUNING=1 MLT_L0_MFMA32=1; A/B).
// XS (the five-stage 16x16x32 form only; layer0_stream_xs_kernel): S5 hands layer1_stream_xs_kernel the INPUT of layer1's projection shortcut instead of
// its output -- xs[Y][X][0..31] = out[2Y][2X][.], [n][32][32][32] fp16 in the first half of the sc buffer -- and that kernel's loader waves run the
// shortcut's K = 32 product (mlt_layer1_kernel.inc).  The centre tap's activation fragment of pixel half hf that S5 re-read for the shortcut IS 16 bytes of
// xs per lane (lane (p16, g4): channels 8 g4 .. 8 g4 + 7 of out[2Y][2 (16 hf + p16)]): S5 wave cb stores half hf = cb, one coalesced 1 KiB store per row, and
// the shortcut's weight reads, MFMAs, epilogue and W5 are gone.  64 KiB per CU leave the chip instead of 128 KiB, and 64 instead of 128 come back.
template <bool F5, bool M16, bool XS>
__device__ __forceinline__ void layer0_stream_body(const Layer0Args &a) {
  static_assert(!XS || (F5 && M16), "the xs hand-off exists for the five-stage 16x16x32 form");
  constexpr int PS = 80, RW = 66, ROWB = RW * PS;                // map rows: zero pixel, 64 pixels, zero pixel
  constexpr int NRT = F5 ? 6 : 8, NRB = 8, NRU = F5 ? 6 : 8, NRO = F5 ? 6 : 0;  // ring slots per map (live rows: 6 / 8 / 6 / 6)
  constexpr int RP = 136, RAWB = RP * 4, NRAW = 16;              // raw rows: 4 zero dwords, 128 (org, |org - pred|) fp16 pairs, 4 zero dwords
  typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Tr = smem, *Br = Tr + NRT * ROWB, *Ur = Br + NRB * ROWB, *Or = Ur + NRU * ROWB, *Z = Or + NRO * ROWB;
  char *Raw = Z + ROWB, *RawZ = Raw + NRAW * RAWB;
  float *BL = (float *)(RawZ + RAWB);   // [0,32) bn1; [32,64) bn2 + shortcut bn; [64,96) layer0.1 bn1; [96,128) layer0.1 bn2; F5: [128,192) layer1.0 bn1, [192,256) its shortcut bn
  constexpr int NBL = F5 ? 256 : 128;
  char *WB = (char *)(BL + NBL);        // 2 border k-steps (7, 8) + 2 shortcut k-steps (5, 6) of the composed first layer: 4 KiB
  int *FL = (int *)(WB + 4096);         // flat-content statistic of the CUs in flight (even / odd CU of the workgroup)
  char *W5 = (char *)(FL + 4);          // F5: the shortcut k-steps of layer1.0 (tap 9), [cout block][k-step] 1 KiB each
  constexpr int ZERO_BYTES = (NRT + NRB + NRU + NRO + 1) * ROWB + (NRAW + 1) * RAWB;
  static_assert(ZERO_BYTES % 16 == 0 && (F5 ? MLT_L0F_LDS_BYTES : MLT_L0_LDS_BYTES) == ZERO_BYTES + NBL * 4 + 4096 + 16 + (F5 ? 4096 : 0), "LDS layout");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // roles: stage 0..3 = S1..S4, 4 = S5.  F5: waves 0, 1 = S1 of the left / right half (both row parities), waves 2, 3 = S5 of couts 0-31 / 32-63
  const int stage = F5 ? (wave < 2 ? 0 : wave < 4 ? 4 : wave >> 2) : CFG_L0_MAP ? wave & 3 : wave >> 2;
  const int unit = F5 ? wave & 3 : CFG_L0_MAP ? wave >> 2 : wave & 3;
  const int par = unit >> 1, blk = (F5 && stage == 0) ? wave : unit & 1;
  const int p = lane & 31, h = lane >> 5, x = 32 * blk + p;      // this lane's pixel of the row
  const int p16 = lane & 15, g4 = lane >> 4, x16 = 32 * blk + p16; // M16: pixel of a 16-pixel half (x16, x16 + 16) / channel group of 8 (B), cout of a 16-cout block / k group (A)
  if ((int)blockIdx.x >= a.n) return;
  if (CFG_L0_PRIO == 1) { if (stage == 0) __builtin_amdgcn_s_setprio(3); else if (stage == 1) __builtin_amdgcn_s_setprio(2); else if (stage == 2) __builtin_amdgcn_s_setprio(1); }
  if (CFG_L0_PRIO == 2) { if (stage == 3) __builtin_amdgcn_s_setprio(3); else if (stage == 2) __builtin_amdgcn_s_setprio(2); else if (stage == 1) __builtin_amdgcn_s_setprio(1); }
  if (CFG_L0_PRIO == 3) { if (stage == 0) __builtin_amdgcn_s_setprio(3); }
  const int nloc = (a.n - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;  // CUs of this workgroup: blockIdx.x + c * gridDim.x
  const int rows_total = 64 * nloc, ksteps = 32 * nloc + (F5 ? 6 : 5);
  for (int o = tid * 16; o < ZERO_BYTES; o += 1024 * 16) *(uint4v *)(smem + o) = uint4v{0u, 0u, 0u, 0u};
  if (tid < 2) FL[tid] = 0;
  if (tid < 32) {
    BL[tid] = a.bias[tid];
    BL[32 + tid] = a.bias2[tid] + a.bias_sc[tid];
    BL[64 + tid] = a.bias3[tid];
    BL[96 + tid] = a.bias4[tid];
    if constexpr (F5) {
      BL[128 + tid] = a.bias5[tid]; BL[160 + tid] = a.bias5[32 + tid];
      if constexpr (!XS) { BL[192 + tid] = a.bias5_sc[tid]; BL[224 + tid] = a.bias5_sc[32 + tid]; }
    }
  }
  if (wave < 4) *(uint4v *)(WB + wave * 1024 + lane * 16) = *(const uint4v *)((const char *)a.w + ((wave < 2 ? 7 : 3) + wave) * 1024 + lane * 16);
  if (F5 && !XS && wave >= 4 && wave < 8) {   // W5[cb][ks] = A fragment of (tap 9, ks, cb)
    const int cb = (wave - 4) >> 1, ks = (wave - 4) & 1;
    *(uint4v *)(W5 + (cb * 2 + ks) * 1024 + lane * 16) = *(const uint4v *)((const char *)a.w5 + ((18 + ks) * 2 + cb) * 1024 + lane * 16);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  auto read16 = [&](const char *row, int dword_index) -> half8 {  // 16 contiguous bytes at an 8-byte aligned LDS address
    const uint2v lo = *(const uint2v *)(row + 4 * dword_index), hi = *(const uint2v *)(row + 4 * dword_index + 8);
    uint4v v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
    return *(half8 *)&v;
  };
  auto raw_row = [&](int c, int y) -> const char * { return (y >= 0 && y < 128) ? Raw + ((128 * c + y) & (NRAW - 1)) * RAWB : RawZ; };
  auto slot_of = [&](auto nrc, int g) -> int {  // ring slot of row g (g >= 0 wherever the result is used)
    constexpr int NRr = decltype(nrc)::value;
    if constexpr (NRr == 8) return g & 7;
    else return g - NRr * (int)__umulhi((uint32_t)g, (uint32_t)(0xFFFFFFFFu / NRr + 1));
  };
  auto map_row = [&](char *ring, auto nrc, int g, int r) -> const char * { return (r >= 0 && r < 64) ? ring + slot_of(nrc, g) * ROWB : Z; };
  constexpr std::integral_constant<int, NRT> nrt{};
  constexpr std::integral_constant<int, NRB> nrb{};
  constexpr std::integral_constant<int, NRU> nru{};
  constexpr std::integral_constant<int, NRO ? NRO : 8> nro{};
  // One 32-pixel block of a 3x3 conv over three map rows; weights in registers, activation fragments PD items ahead.  The reads are issued from
  // inline asm with counted waits: written in C++ the compiler regroups them into pairs -- read 2, wait for both, 2 MFMAs -- whatever PD says, and a
  // wave then spends nine LDS round trips per row (the first form of this kernel: 0.87 ms, MFMA knocked out 0.63).  The four bias quads of the
  // epilogue are read into the fragment registers the last PD items free (same size, no extra VGPRs), so they land under the last MFMAs.
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  auto lds_of = [&](const char *q) -> uint32_t { return lds0 + (uint32_t)(q - smem); };
  // (S2 folds its bias into the shortcut sum before the conv and runs one fragment less in flight -- pdc = PD - 1, bc = false: its two accumulators
  // leave no room; with four in flight one of its weight fragments was reloaded from scratch every row)
  // Across the barrier (CFG_L0_XPRE): the row ABOVE the next row of this wave is complete before the step ends, so its first PD fragments are
  // requested behind the epilogue's stores -- the barrier waits with lgkmcnt(PD), LDS operations of a wave complete in order -- and the next step
  // starts with MFMAs instead of sixteen waves' first LDS round trips.  `pre` says that this has happened for the row at hand.
  auto conv18 = [&](const half8 (&wf)[18], auto &bf, bool pre, const char *rm, const char *r0, const char *rp, int bias_off, float4v (&bq)[4], auto pdc, auto bc) -> float16v {
    constexpr int PD = decltype(pdc)::value;
    constexpr bool BIAS = decltype(bc)::value;
    const int lo = x * PS + h * 16;
    const uint32_t rows[3] = {lds_of(rm) + lo, lds_of(r0) + lo, lds_of(rp) + lo};
    const uint32_t ba = BIAS ? lds_of((const char *)(BL + bias_off + 4 * h)) : 0u;
    static_assert(PD <= 6 && (!BIAS || PD >= 4), "the first PD items lie in one row; bias quads ride in the last four fragment slots");
    auto rd = [&](auto itc) {
      constexpr int item = decltype(itc)::value, tp = item >> 1, ks = item & 1, dy = tp / 3, dx = tp - dy * 3;
      if constexpr (CFG_L0_KO & 1) bf[item % PD] = wf[item];
      else lds_read128<dx * PS + ks * 32>(bf[item % PD], rows[dy]);
    };
    if (!pre) static_for<PD>([&](auto ic) { rd(ic); });
    float16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    static_for<18>([&](auto itc) {
      constexpr int item = decltype(itc)::value;
      constexpr int frags_behind = (17 - item) < (PD - 1) ? (17 - item) : (PD - 1);       // younger fragment reads in flight
      constexpr int bias_behind = !BIAS ? 0 : item - (18 - PD) > 0 ? (item - (18 - PD) < 4 ? item - (18 - PD) : 4) : 0;  // bias quads issued so far (all younger)
      if constexpr (!(CFG_L0_KO & 1)) { lds_wait<frags_behind + bias_behind>(); lds_touch(bf[item % PD]); }
      if (CFG_L0_KO & 2) asm volatile("" ::"v"(bf[item % PD]), "v"(wf[item]));
      else acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[item], bf[item % PD], acc, 0, 0, 0);
      if constexpr (item + PD < 18) rd(std::integral_constant<int, item + PD>{});
      else if constexpr (BIAS && item - (18 - PD) < 4) lds_read128<(item - (18 - PD)) * 32>(bf[item % PD], ba);  // bias quad q = item - (18 - PD): BL[bias_off + 4h + 8q ..]
    });
    if (CFG_L0_KO & 2) asm volatile("" : "+v"(acc));
    if constexpr (BIAS) {
      lds_wait<0>();
      static_for<4>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        lds_touch(bf[(18 - PD + q) % PD]);
        bq[q] = *(const float4v *)&bf[(18 - PD + q) % PD];
      });
    }
    return acc;
  };
  auto prefetch_row = [&](auto &bf, const char *rm, auto pdc) {  // items 0 .. PD-1 of the next row's conv: all of them taps of the row above it
    constexpr int PD = decltype(pdc)::value;
    if constexpr (M16) {
      const uint32_t row = lds_of(rm) + x16 * PS + g4 * 16;
      static_for<PD>([&](auto ic) {
        constexpr int item = decltype(ic)::value, dx = item >> 1, hf = item & 1;
        lds_read128<(dx + 16 * hf) * PS>(bf[item], row);
      });
      return;
    }
    const uint32_t row = lds_of(rm) + x * PS + h * 16;
    static_for<PD>([&](auto ic) {
      constexpr int item = decltype(ic)::value, dx = item >> 1, ks = item & 1;
      lds_read128<dx * PS + ks * 32>(bf[item], row);
    });
  };
  auto load_wf = [&](half8 (&wf)[18], const void *w) {
#pragma unroll
    for (int i = 0; i < 18; ++i) wf[i] = *(const half8 *)((const char *)w + i * 1024 + lane * 16);
#pragma unroll
    for (int i = 0; i < 18; ++i) asm volatile("" ::"v"(wf[i]));  // first use in front of the row loop (no vmcnt(0) inside it)
  };
  auto store_row = [&](char *ring, auto nrc, int g, const half4 (&o)[4]) {  // 16-byte stores: lanes 0-31 take channels 16qq..+7, lanes 32-63 the next 8
    char *dst = ring + slot_of(nrc, g) * ROWB + (x + 1) * PS + 16 * h;
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) *(uint4v *)(dst + 32 * qq) = pair16(o[2 * qq], o[2 * qq + 1]);
  };
  // ---- 16x16x32 forms (M16) of the helpers above.  Fragment 2 tap + c of a conv: couts 16 c .. 16 c + 15, the tap's 32 input channels; lane (i, g) holds
  // W[cout 16 c + i][cin 8 g .. 8 g + 7] = the 32x32x16 packing's fragment of k16 step 2 tap + (g >> 1), lane (g & 1) * 32 + 16 c + i (istride: bytes between
  // k16 steps of the packed weights).  Item j = 2 tap + hf of a row: activation fragment of pixels x16 + 16 hf (+ dx), all 32 channels; two MFMAs per item.
  // acc[c][hf][e] = cout 16 c + 4 g + e of pixel x16 + 16 hf.
  auto load_wf_m = [&](half8 (&wf)[18], const char *w, int istride) {
#pragma unroll
    for (int i = 0; i < 18; ++i) wf[i] = *(const half8 *)(w + (size_t)((i & ~1) + (g4 >> 1)) * istride + ((g4 & 1) * 32 + 16 * (i & 1) + p16) * 16);
#pragma unroll
    for (int i = 0; i < 18; ++i) asm volatile("" ::"v"(wf[i]));
  };
  auto conv18m = [&](const half8 (&wf)[18], auto &bf, bool pre, const char *rm, const char *r0, const char *rp, int bias_off, float4v (&bq)[2], auto pdc, auto bc, float4v (&acc)[2][2]) {
    constexpr int PD = decltype(pdc)::value;
    constexpr bool BIAS = decltype(bc)::value;
    const int lo = x16 * PS + g4 * 16;
    const uint32_t rows[3] = {lds_of(rm) + lo, lds_of(r0) + lo, lds_of(rp) + lo};
    const uint32_t ba = BIAS ? lds_of((const char *)(BL + bias_off + 4 * g4)) : 0u;
    static_assert(PD <= 6 && (!BIAS || PD >= 2), "the first PD items lie in one row; the two bias quads ride in the last fragment slots");
    auto rd = [&](auto itc) {
      constexpr int item = decltype(itc)::value, tp = item >> 1, hf = item & 1, dy = tp / 3, dx = tp - dy * 3;
      lds_read128<(dx + 16 * hf) * PS>(bf[item % PD], rows[dy]);
    };
    if (!pre) static_for<PD>([&](auto ic) { rd(ic); });
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q >> 1][q & 1] = float4v{0.f, 0.f, 0.f, 0.f};
    static_for<18>([&](auto itc) {
      constexpr int item = decltype(itc)::value, tp = item >> 1, hf = item & 1;
      constexpr int frags_behind = (17 - item) < (PD - 1) ? (17 - item) : (PD - 1);
      constexpr int bias_behind = !BIAS ? 0 : item - (18 - PD) > 0 ? (item - (18 - PD) < 2 ? item - (18 - PD) : 2) : 0;
      lds_wait<frags_behind + bias_behind>();
      lds_touch(bf[item % PD]);
      acc[0][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * tp], bf[item % PD], acc[0][hf], 0, 0, 0);
      acc[1][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * tp + 1], bf[item % PD], acc[1][hf], 0, 0, 0);
      if constexpr (item + PD < 18) rd(std::integral_constant<int, item + PD>{});
      else if constexpr (BIAS && item - (18 - PD) < 2) lds_read128<(item - (18 - PD)) * 64>(bf[item % PD], ba);  // bias quad of cout block c = item - (18 - PD): BL[bias_off + 16 c + 4 g ..]
    });
    if constexpr (BIAS) {
      lds_wait<0>();
      static_for<2>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        lds_touch(bf[(18 - PD + c) % PD]);
        bq[c] = *(const float4v *)&bf[(18 - PD + c) % PD];
      });
    }
  };
  auto store_row_m = [&](char *ring, auto nrc, int g, const half4 (&o)[2][2]) {  // 8-byte stores: 4 consecutive channels of a pixel per lane and block
    char *dst = ring + slot_of(nrc, g) * ROWB + (x16 + 1) * PS + 8 * g4;
#pragma unroll
    for (int q = 0; q < 4; ++q) *(half4 *)(dst + 32 * (q >> 1) + 16 * PS * (q & 1)) = o[q >> 1][q & 1];
  };
#ifdef MLT_PHASE_TIMING
#define L0_PH_FLUSH() do { if (lane == 0 && unit == 0 && stage < 4) { for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_phase_l0[stage][i_], ph_acc[i_]); } } while (0)
#else
#define L0_PH_FLUSH()
#endif
#define L0_STEP_END_PRE(n) asm volatile("s_waitcnt lgkmcnt(%0)\n\ts_barrier" ::"n"(n) : "memory")
#define L0_STEP_END() do { if (CFG_L0_KO & 8) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); } while (0)
  // end of a conv stage's step: request the next row's first fragments (when there is a next row), then wait for the stores and meet the others
  auto step_end = [&](auto &bf, bool &pre, char *ring, auto nrc, int g_next, auto pdc) {
    constexpr int PD = decltype(pdc)::value;
    if (CFG_L0_XPRE && !(CFG_L0_KO & 9) && g_next >= 0 && g_next < rows_total) {
      prefetch_row(bf, map_row(ring, nrc, g_next - 1, (g_next & 63) - 1), pdc);
      pre = true;
      L0_STEP_END_PRE(PD);
    } else {
      pre = false;
      L0_STEP_END();
    }
  };

  if (stage == 0) {
    // ================= S1: raw rows in, t rows out =================
    half8 am[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) am[k] = *(const half8 *)((const char *)a.w + k * 1024 + lane * 16);
#pragma unroll
    for (int k = 0; k < 5; ++k) asm volatile("" ::"v"(am[k]));
    // raw row G of the workgroup = row G & 127 of its CU G >> 7: one wave fetches one row per step as 32 quads of 4 pixels (lanes 32-63 mirror
    // lanes 0-31 and store nothing; F5: two rows per wave, lanes 32-63 the second).  issue (global -> registers) long before commit (convert, registers -> LDS): with one step between them every
    // step waited for a dependent HBM access (knock-outs: 1.2 us per step whatever the stages did).  The step loop runs in groups of RD steps: the
    // rows a group commits were issued during the first half of the PREVIOUS group (the compiler drains vmcnt at the loop head -- by then the
    // youngest load is RD / 2 steps old) and change registers at the group's end.
    constexpr int RD = CFG_L0_RD;
    static_assert(RD % 2 == 0, "RD");
    uint2v vo[RD], vp[RD], no[RD], np[RD];
    const int rsel = F5 ? 2 * wave + h : unit;     // which of the step's four raw rows this lane fetches
    const bool rlane = F5 || h == 0;               // ... and whether it is the lane that converts and stores it
    auto issue = [&](uint2v &o2, uint2v &p2, int G) {  // (unconditional -- rows behind the last CU re-load its last row -- so that the waits can be counted)
      G = G < 128 * nloc ? G : 128 * nloc - 1;
      const int c = G >> 7, y = G & 127;
      const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
      o2 = *(const uint2v *)(a.org + n * a.org_cu_stride + (size_t)y * a.org_row_stride + 4 * p);
      p2 = *(const uint2v *)(a.pred + n * a.pred_cu_stride + (size_t)y * a.pred_row_stride + 4 * p);
    };
    auto commit = [&](const uint2v &o2, const uint2v &p2, int G, bool live = true) {
      live = live && rlane && G < 128 * nloc;      // (per lane when F5: the two halves of a wave hold different rows)
      uint4v w;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int16_t o = (int16_t)(o2[jj >> 1] >> (16 * (jj & 1))), q = (int16_t)(p2[jj >> 1] >> (16 * (jj & 1)));
        w[jj] = prep_pair(o, q);
      }
      if (a.flat) {  // flat-content guard statistic: every quad of the CU exactly once (flat_stat_kernel's count)
        const int fb = live ? quad_flat_bits(w[0], w[1], w[2], w[3]) : 0;
        const unsigned long long b1 = __ballot(fb & 1), b2 = __ballot(fb & 2);   // per half-wave: its 32 lanes hold one row
        const int nflat = __builtin_popcount((unsigned)(h ? b1 >> 32 : b1)) + (__builtin_popcount((unsigned)(h ? b2 >> 32 : b2)) << MLT_FLAT_EXACT_SHIFT);
        if (nflat && p == 0 && live) atomicAdd(FL + ((G >> 7) & 1), nflat);  // LDS; S4 hands the CU's sum to a.flat with its last row (no vector-memory op here)
      }
      if (live) *(uint4v *)(Raw + (G & (NRAW - 1)) * RAWB + 16 + 16 * p) = w;
    };
    issue(vo[0], vp[0], rsel); commit(vo[0], vp[0], rsel);            // rows 0-3
    if (unit == 0) { issue(vo[0], vp[0], 4); commit(vo[0], vp[0], 4, h == 0); }
#pragma unroll
    for (int d = 0; d < RD; ++d) issue(vo[d], vp[d], 4 * d + 5 + rsel);  // rows 4k + 5 .. 4k + 8 are committed in step k and read from step k + 1 on
    L0_STEP_END();
    PH_DECL;
    for (int k0 = 0; k0 < ksteps; k0 += RD) { static_for<RD>([&](auto slc) {
      constexpr int sl = decltype(slc)::value;
      const int k = k0 + sl;
      if (k >= ksteps) return;
      PH_MARK(3);
      commit(vo[sl], vp[sl], 4 * k + 5 + rsel);
      if constexpr (sl < RD / 2) {
        issue(no[2 * sl], np[2 * sl], 4 * (k0 + RD + 2 * sl) + 5 + rsel);
        issue(no[2 * sl + 1], np[2 * sl + 1], 4 * (k0 + RD + 2 * sl + 1) + 5 + rsel);
      }
      PH_MARK(0);
#pragma unroll
      for (int u = 0; u < (F5 ? 2 : 1); ++u) {
      const int g = 2 * k + (F5 ? u : par);
      if (g < rows_total) {
        const int c = g >> 6, r = g & 63;
        half8 bk[5];
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) bk[dy] = read16(raw_row(c, 2 * r - 2 + dy), 2 * x + 2 + 4 * h);  // window origin = input (2r-2, 2x-2); this lane: columns +4h .. +4h+3
        float16v acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(am[dy], bk[dy], acc, 0, 0, 0);
        // border corrections (conv1 pads the STEM map, the composed conv the INPUT): output row 0 / column 0 only
        if (r == 0 || blk == 0) {
          const bool topb = r == 0, leftb = x == 0;
          if (blk == 0) {  // Left[u] x in(2r-2+u, 0) = window (dy = u, dx = 2); Corner x in(0, 0)
            const uint32_t l4 = *(const uint32_t *)(raw_row(c, 2 * r + 2) + 16), c0 = *(const uint32_t *)(raw_row(c, 0) + 16);
            uint4v bb;
            if (h == 0) {
              bb[0] = ((const uint32_t *)&bk[0])[2]; bb[1] = ((const uint32_t *)&bk[1])[2];
              bb[2] = ((const uint32_t *)&bk[2])[2]; bb[3] = ((const uint32_t *)&bk[3])[2];
            } else {
              bb[0] = l4; bb[1] = topb ? c0 : 0u; bb[2] = 0u; bb[3] = 0u;
            }
            if (!leftb) bb = uint4v{0u, 0u, 0u, 0u};
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8 *)(WB + lane * 16), *(half8 *)&bb, acc, 0, 0, 0);
          }
          if (topb) {  // Top[v] x in(0, 2x-2+v) = window (dy = 2, dx = v)
            uint4v bb = *(const uint4v *)&bk[2];
            if (h == 1) { bb[1] = 0u; bb[2] = 0u; bb[3] = 0u; }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8 *)(WB + 1024 + lane * 16), *(half8 *)&bb, acc, 0, 0, 0);
          }
        }
        PH_MARK(1);
        half4 ov[4];
        static_for<4>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          const float4v b1q = *(const float4v *)(BL + 4 * h + 8 * q);
          const half4 none{};
          ov[q] = act_quad<q>(acc, a.acc_scale, b1q, false, none, true);  // relu(acc * scale + bias), packed arithmetic
        });
        store_row(Tr, nrt, g, ov);
        PH_MARK(2);
      }
      }
      L0_STEP_END();
    });
#pragma unroll
      for (int d = 0; d < RD; ++d) { vo[d] = no[d]; vp[d] = np[d]; }
    }
    L0_PH_FLUSH();
  } else if (stage == 1) {
    // ================= S2: b0 = relu(conv2(t) + shortcut) =================
    half8 wf[18], bf[CFG_L0_PD - 1];
    bool pre = false;
    constexpr std::integral_constant<int, CFG_L0_PD - 1> pdc{};
    if constexpr (M16) load_wf_m(wf, (const char *)a.w2, 1024); else load_wf(wf, a.w2);
    L0_STEP_END();
    PH_DECL;
    for (int k = 0; k < ksteps; ++k) {
      PH_MARK(3);
      const int g = 2 * k + par - 3;
      if constexpr (M16) {
        if (g >= 0 && g < rows_total) {
          const int c = g >> 6, r = g & 63;
          // shortcut: ONE k = 32 step = round 5's k-steps 5 | 6.  B: lane (pixel, g): g >> 1 = 0: k-step 5, where lane half g & 1 = 0 / 1 reads row by = 0 / 1;
          // g >> 1 = 1: k-step 6, row by = 2 (its upper half carries zero weights).  A: the two k-steps' fragments in WB, gathered for the 16-cout blocks.
          const char *s0 = (g4 >> 1) ? raw_row(c, 2 * r + 1) : (g4 & 1) ? raw_row(c, 2 * r) : raw_row(c, 2 * r - 1);
          const uint32_t wa = lds_of(WB + 2048 + (g4 >> 1) * 1024 + ((g4 & 1) * 32 + p16) * 16);
          float4v accs[2][2];
          {
            // (the weight fragments through asm reads: as plain loads they are loop-invariant, the compiler hoists them out of the row loop and then
            // spills them -- three 16-byte scratch reloads per row in the four-stage form)
            half8 a0, a1;
            lds_read128<0>(a0, wa);
            lds_read128<256>(a1, wa);
            const half8 sb0 = read16(s0, 2 * x16 + 2), sb1 = read16(s0, 2 * (x16 + 16) + 2);
            lds_wait<0>();
            lds_touch(a0); lds_touch(a1);
            const float4v z4 = {0.f, 0.f, 0.f, 0.f};
            accs[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, sb0, z4, 0, 0, 0);
            accs[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, sb0, z4, 0, 0, 0);
            accs[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, sb1, z4, 0, 0, 0);
            accs[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, sb1, z4, 0, 0, 0);
          }
          static_for<2>([&](auto cc) {  // shortcut * scale + bias now (the bias registers are free again before the conv starts)
            constexpr int cq = decltype(cc)::value;
            const float4v bq = *(const float4v *)(BL + 32 + 16 * cq + 4 * g4);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
              for (int ep = 0; ep < 2; ++ep) {
                const float2v s2 = {accs[cq][hf][2 * ep], accs[cq][hf][2 * ep + 1]}, b2 = {bq[2 * ep], bq[2 * ep + 1]};
                const float2v y2 = s2 * a.acc_scale + b2;
                accs[cq][hf][2 * ep] = y2[0]; accs[cq][hf][2 * ep + 1] = y2[1];
              }
          });
          float4v bqs[2], acc[2][2];
          PH_MARK(0);
          conv18m(wf, bf, pre, map_row(Tr, nrt, g - 1, r - 1), map_row(Tr, nrt, g, r), map_row(Tr, nrt, g + 1, r + 1), 32, bqs, pdc, std::false_type{}, acc);
          half4 hq[2][2];
          PH_MARK(1);
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int ep = 0; ep < 2; ++ep) {  // relu(conv2 + (shortcut * scale + bias)), the sum in fp32, packed arithmetic
              const float2v c2 = {acc[q >> 1][q & 1][2 * ep], acc[q >> 1][q & 1][2 * ep + 1]}, y2 = {accs[q >> 1][q & 1][2 * ep], accs[q >> 1][q & 1][2 * ep + 1]};
              const float2v x2 = c2 + y2;
              half2v h2 = __builtin_convertvector(x2, half2v);
              h2 = __builtin_elementwise_max(h2, (half2v){(_Float16)0, (_Float16)0});
              hq[q >> 1][q & 1][2 * ep] = h2[0];
              hq[q >> 1][q & 1][2 * ep + 1] = h2[1];
            }
          store_row_m(Br, nrb, g, hq);
          PH_MARK(2);
        }
        step_end(bf, pre, Tr, nrt, g + 2, pdc);
        continue;
      }
      if (g >= 0 && g < rows_total) {
        const int c = g >> 6, r = g & 63;
        // shortcut taps (by, bx) at input (2r+by-1, 2x+bx-1): lanes h = 0 / 1 read rows by = 0 / 1 (k-step 5), every lane row by = 2 (k-step 6, upper
        // half: zero weights), columns 2x-2 .. 2x+1 (the first one carries a zero weight)
        const char *s0 = h ? raw_row(c, 2 * r) : raw_row(c, 2 * r - 1);
        const half8 sb0 = read16(s0, 2 * x + 2), sb1 = read16(raw_row(c, 2 * r + 1), 2 * x + 2);
        float16v accs;
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[i] = 0.f;
        accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8 *)(WB + 2048 + lane * 16), sb0, accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const half8 *)(WB + 3072 + lane * 16), sb1, accs, 0, 0, 0);
        static_for<4>([&](auto qc) {  // shortcut * scale + bias now: the bias registers are free again before the conv starts
          constexpr int q = decltype(qc)::value;
          const float4v bq = *(const float4v *)(BL + 32 + 4 * h + 8 * q);
#pragma unroll
          for (int ep = 0; ep < 2; ++ep) {
            const float2v s2 = {accs[4 * q + 2 * ep], accs[4 * q + 2 * ep + 1]}, b2 = {bq[2 * ep], bq[2 * ep + 1]};
            const float2v y2 = s2 * a.acc_scale + b2;
            accs[4 * q + 2 * ep] = y2[0]; accs[4 * q + 2 * ep + 1] = y2[1];
          }
        });
        float4v bqs[4];
        PH_MARK(0);
        const float16v acc = conv18(wf, bf, pre, map_row(Tr, nrt, g - 1, r - 1), map_row(Tr, nrt, g, r), map_row(Tr, nrt, g + 1, r + 1), 32, bqs, pdc, std::false_type{});
        half4 hq[4];
        PH_MARK(1);
        if (CFG_L0_KO & 4) { asm volatile("" ::"v"(acc), "v"(accs)); step_end(bf, pre, Tr, nrt, g + 2, pdc); continue; }
        static_for<4>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
#pragma unroll
          for (int ep = 0; ep < 2; ++ep) {  // relu(conv2 + (shortcut * scale + bias)), the sum in fp32, packed arithmetic
            const float2v c2 = {acc[4 * q + 2 * ep], acc[4 * q + 2 * ep + 1]}, y2 = {accs[4 * q + 2 * ep], accs[4 * q + 2 * ep + 1]};
            const float2v x2 = c2 + y2;
            half2v h2 = __builtin_convertvector(x2, half2v);
            h2 = __builtin_elementwise_max(h2, (half2v){(_Float16)0, (_Float16)0});
            hq[q][2 * ep] = h2[0];
            hq[q][2 * ep + 1] = h2[1];
          }
        });
        store_row(Br, nrb, g, hq);
        PH_MARK(2);
      }
      step_end(bf, pre, Tr, nrt, g + 2, pdc);
    }
    L0_PH_FLUSH();
  } else if (stage == 2) {
    // ================= S3: u = relu(bn(conv1'(b0))) =================
    half8 wf[18], bf[CFG_L0_PD];
    bool pre = false;
    constexpr std::integral_constant<int, CFG_L0_PD> pdc{};
    if constexpr (M16) load_wf_m(wf, (const char *)a.w3, 1024); else load_wf(wf, a.w3);
    L0_STEP_END();
    PH_DECL;
    for (int k = 0; k < ksteps; ++k) {
      PH_MARK(3);
      const int g = 2 * k + par - 6;
      if constexpr (M16) {
        if (g >= 0 && g < rows_total) {
          const int r = g & 63;
          float4v bqs[2], acc[2][2];
          PH_MARK(0);
          conv18m(wf, bf, pre, map_row(Br, nrb, g - 1, r - 1), map_row(Br, nrb, g, r), map_row(Br, nrb, g + 1, r + 1), 64, bqs, pdc, std::true_type{}, acc);
          half4 o[2][2];
          PH_MARK(1);
          const half4 none{};
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q >> 1][q & 1] = act_quad<0>(acc[q >> 1][q & 1], 1.f, bqs[q >> 1], false, none, true);
          store_row_m(Ur, nru, g, o);
          PH_MARK(2);
        }
        step_end(bf, pre, Br, nrb, g + 2, pdc);
        continue;
      }
      if (g >= 0 && g < rows_total) {
        const int r = g & 63;
        float4v bqs[4];
        PH_MARK(0);
        const float16v acc = conv18(wf, bf, pre, map_row(Br, nrb, g - 1, r - 1), map_row(Br, nrb, g, r), map_row(Br, nrb, g + 1, r + 1), 64, bqs, pdc, std::true_type{});
        half4 o[4];
        PH_MARK(1);
        if (CFG_L0_KO & 4) { asm volatile("" ::"v"(acc)); step_end(bf, pre, Br, nrb, g + 2, pdc); continue; }
        if constexpr (CFG_L0_PKEPI) {
          static_for<4>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const half4 none{};
            o[q] = act_quad<q>(acc, 1.f, bqs[q], false, none, true);
          });
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4v bq = bqs[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[q][e] = (_Float16)fmaxf(acc[4 * q + e] + bq[e], 0.f);
          }
        }
        store_row(Ur, nru, g, o);
        PH_MARK(2);
      }
      step_end(bf, pre, Br, nrb, g + 2, pdc);
    }
    L0_PH_FLUSH();
  } else if (stage == 3) {
    // ================= S4: out = relu(bn(conv2'(u)) + b0) -> HBM (F5: -> S5's ring) =================
    half8 wf[18], bf[CFG_L0_PD];
    bool pre = false;
    constexpr std::integral_constant<int, CFG_L0_PD> pdc{};
    if constexpr (M16) load_wf_m(wf, (const char *)a.w4, 1024); else load_wf(wf, a.w4);
    L0_STEP_END();
    PH_DECL;
    for (int k = 0; k < ksteps; ++k) {
      PH_MARK(3);
      const int g = 2 * k + par - 9;
      if constexpr (M16) {
        if (g >= 0 && g < rows_total) {
          const int c = g >> 6, r = g & 63;
          float4v bqs[2], acc[2][2];
          PH_MARK(0);
          conv18m(wf, bf, pre, map_row(Ur, nru, g - 1, r - 1), map_row(Ur, nru, g, r), map_row(Ur, nru, g + 1, r + 1), 96, bqs, pdc, std::true_type{}, acc);
          const char *rsrc = Br + slot_of(nrb, g) * ROWB + (x16 + 1) * PS + 8 * g4;  // residual: this row of b0, 8-byte reads
          half4 hq[2][2];
          PH_MARK(1);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const half4 rr = *(const half4 *)(rsrc + 32 * (q >> 1) + 16 * PS * (q & 1));
            hq[q >> 1][q & 1] = act_quad<0>(acc[q >> 1][q & 1], 1.f, bqs[q >> 1], true, rr, true);
          }
          const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
          if (a.flat && r == 63 && blk == 0 && lane == 0) {  // S1 finished this CU's statistic ~30 steps ago and will not touch the slot before CU c + 2
            const int v = FL[c & 1];
            FL[c & 1] = 0;
            if (v) atomicAdd(a.flat + n, v);
          }
          if constexpr (F5) store_row_m(Or, nro, g, hq);
          else {
            char *cu_out = (char *)a.y + n * (size_t)(64 * 64 * 32 * 2);
            const uint32_t ob = (uint32_t)(((r * 64 + x16) * 32 + 4 * g4) * 2);
#pragma unroll
            for (int q = 0; q < 4; ++q) *(half4 *)(cu_out + ob + 32 * (q >> 1) + 16 * 64 * (q & 1)) = hq[q >> 1][q & 1];
          }
        }
        PH_MARK(2);
        step_end(bf, pre, Ur, nru, g + 2, pdc);
        continue;
      }
      if (g >= 0 && g < rows_total) {
        const int c = g >> 6, r = g & 63;
        float4v bqs[4];
        PH_MARK(0);
        const float16v acc = conv18(wf, bf, pre, map_row(Ur, nru, g - 1, r - 1), map_row(Ur, nru, g, r), map_row(Ur, nru, g + 1, r + 1), 96, bqs, pdc, std::true_type{});
        const char *rsrc = Br + slot_of(nrb, g) * ROWB + (x + 1) * PS + 16 * h;  // residual: this row of b0, 16-byte reads
        half4 hq[4];
        PH_MARK(1);
        if (CFG_L0_KO & 4) { asm volatile("" ::"v"(acc)); step_end(bf, pre, Ur, nru, g + 2, pdc); continue; }
        static_for<2>([&](auto qc) {
          constexpr int qq = decltype(qc)::value;
          half4 rr[2];
          unpair16(*(const uint4v *)(rsrc + 32 * qq), rr[0], rr[1]);
          if constexpr (CFG_L0_PKEPI) {
            hq[2 * qq] = act_quad<2 * qq>(acc, 1.f, bqs[2 * qq], true, rr[0], true);
            hq[2 * qq + 1] = act_quad<2 * qq + 1>(acc, 1.f, bqs[2 * qq + 1], true, rr[1], true);
          } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
              const float4v bq = bqs[2 * qq + kk];
#pragma unroll
              for (int e = 0; e < 4; ++e) hq[2 * qq + kk][e] = (_Float16)fmaxf(acc[8 * qq + 4 * kk + e] + bq[e] + (float)rr[kk][e], 0.f);
            }
          }
        });
        const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
        if (a.flat && r == 63 && blk == 0 && lane == 0) {  // S1 finished this CU's statistic ~30 steps ago and will not touch the slot before CU c + 2
          const int v = FL[c & 1];
          FL[c & 1] = 0;
          if (v) atomicAdd(a.flat + n, v);
        }
        if constexpr (F5) store_row(Or, nro, g, hq);
        else {
          char *cu_out = (char *)a.y + n * (size_t)(64 * 64 * 32 * 2);            // wave-uniform base (SGPRs) + a 32-bit lane offset
          const uint32_t ob = (uint32_t)(((r * 64 + x) * 32 + 8 * h) * 2);
#pragma unroll
          for (int qq = 0; qq < 2; ++qq) *(uint4v *)(cu_out + ob + 32 * qq) = pair16(hq[2 * qq], hq[2 * qq + 1]);
        }
      }
      PH_MARK(2);
      step_end(bf, pre, Ur, nru, g + 2, pdc);
    }
    L0_PH_FLUSH();
  } else if constexpr (F5) {
    // ================= S5: t1 = relu(bn(conv3x3 stride 2 (out))), sc1 = bn(conv1x1 stride 2 (out)): 32 -> 64 channels, one output row per step =================
    // (conv_mfma_kernel<32, 64, 2, 9, true, ...>: items tap-major, k-step inside; the shortcut is "tap 9" on the centre tap's pixels with its own
    // accumulator; A fragment of (tap, k-step, cout block cb) at ((tap * 2 + ks) * 2 + cb) KiB of the packed weights)
    // The shortcut's two MFMAs run AFTER the conv's eighteen: their operands -- the centre tap's two activation fragments and the shortcut's two
    // weight fragments (LDS, W5) -- are read into the four fragment slots the last items free, so the second accumulator is not live during the conv
    // (with it the wave needed 130 VGPRs and reloaded three weight fragments from scratch per row).
    const int cb = wave - 2;
    constexpr int PD = CFG_L0_PD;
    static_assert(PD == 4, "four slots for the shortcut's four operands");
    half8 wf[18], bf[PD];
    if constexpr (M16) load_wf_m(wf, (const char *)a.w5 + cb * 1024, 2048);
    else {
#pragma unroll
      for (int i = 0; i < 18; ++i) wf[i] = *(const half8 *)((const char *)a.w5 + (i * 2 + cb) * 1024 + lane * 16);
#pragma unroll
      for (int i = 0; i < 18; ++i) asm volatile("" ::"v"(wf[i]));
    }
    const uint32_t wsa = M16 ? lds_of(W5 + cb * 2048 + (g4 >> 1) * 1024 + ((g4 & 1) * 32 + p16) * 16) : lds_of(W5 + cb * 2048 + lane * 16);
    L0_STEP_END();
    for (int k = 0; k < ksteps; ++k) {
      const int G5 = k - 6;                        // output row of the workgroup: row G5 & 31 of CU G5 >> 5; its input rows 2 G5 - 1 .. 2 G5 + 1 left S4 by step k - 1
      if constexpr (M16) {
        if (G5 >= 0 && G5 < 32 * nloc) {
          const int c = G5 >> 5, Y = G5 & 31, g0 = 2 * G5;
          const int lo = (2 * p16) * PS + g4 * 16;   // output pixel 16 hf + p16 reads stored columns 2 (16 hf + p16) + dx
          const uint32_t rows[3] = {lds_of(map_row(Or, nro, g0 - 1, 2 * Y - 1)) + lo, lds_of(Or + slot_of(nro, g0) * ROWB) + lo, lds_of(Or + slot_of(nro, g0 + 1) * ROWB) + lo};
          auto rd = [&](auto itc) {
            constexpr int item = decltype(itc)::value, tp = item >> 1, hf = item & 1, dy = tp / 3, dx = tp - dy * 3;
            lds_read128<(dx + 32 * hf) * PS>(bf[item % PD], rows[dy]);
          };
          static_for<PD>([&](auto ic) { rd(ic); });
          float4v acc[2][2];
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q >> 1][q & 1] = float4v{0.f, 0.f, 0.f, 0.f};
          static_for<18>([&](auto itc) {
            constexpr int item = decltype(itc)::value, tp = item >> 1, hf = item & 1, e = item - (18 - PD);   // e >= 0: extra read number e follows this item
            lds_wait<((17 - item) < (PD - 1) ? (17 - item) : (PD - 1)) + (e > 0 ? (XS ? 1 : e) : 0)>();             // (XS: ONE extra read, behind item 18 - PD)
            lds_touch(bf[item % PD]);
            acc[0][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * tp], bf[item % PD], acc[0][hf], 0, 0, 0);
            acc[1][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * tp + 1], bf[item % PD], acc[1][hf], 0, 0, 0);
            if constexpr (item + PD < 18) rd(std::integral_constant<int, item + PD>{});
            else if constexpr (XS) { if constexpr (e == 0) lds_read128<PS>(bf[item % PD], rows[1] + cb * (32 * PS)); }   // centre tap, pixel half cb: this wave's piece of xs
            else if constexpr (e < 2) lds_read128<(1 + 32 * e) * PS>(bf[item % PD], rows[1]);   // centre tap (dy 1, dx 1), pixel half e
            else lds_read128<(e - 2) * 256>(bf[item % PD], wsa);                                 // shortcut weights, cout block e - 2
          });
          const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
          char *cu_t = (char *)a.y_t + n * (size_t)(32 * 32 * 64 * 2) + (Y * 32 * 64 + cb * 32) * 2;
          char *cu_sc = (char *)a.y_sc + n * (size_t)(32 * 32 * 64 * 2) + (((2 * cb) << 10) + Y * 32) * 32;
          const uint32_t ot = (uint32_t)(p16 * 128 + g4 * 8), os = (uint32_t)(p16 * 32 + g4 * 8);
          const float *bl5 = BL + 128 + 32 * cb + 4 * g4;
          const half4 none{};
#pragma unroll
          for (int q = 0; q < 4; ++q)   // t: NHWC, couts cb * 32 + 16 c + 4 g .. of pixel 16 hf + p16
            *(half4 *)(cu_t + ot + 32 * (q >> 1) + 16 * 128 * (q & 1)) = act_quad<0>(acc[q >> 1][q & 1], a.scale5, *(const float4v *)(bl5 + 16 * (q >> 1)), false, none, true);
          lds_wait<0>();
          if constexpr (XS) {   // xs [n][32][32][32]: row Y, pixels 16 cb .. 16 cb + 15, this lane's 8 channels
            lds_touch(bf[(18 - PD) % PD]);
            *(half8 *)((char *)a.y_sc + n * (size_t)(32 * 32 * 32 * 2) + (Y * 32 + 16 * cb) * 64 + p16 * 64 + g4 * 16) = bf[(18 - PD) % PD];
          } else {
          static_for<PD>([&](auto ic) { lds_touch(bf[decltype(ic)::value]); });
          float4v accs[2][2];
          const float4v z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int q = 0; q < 4; ++q) accs[q >> 1][q & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[(18 - PD + 2 + (q >> 1)) % PD], bf[(18 - PD + (q & 1)) % PD], z4, 0, 0, 0);
#pragma unroll
          for (int q = 0; q < 4; ++q)   // sc chunk-major ([n][64 / 16][32 x 32][16] fp16): chunk 2 cb + c, this lane's channels 4 g .. 4 g + 3
            *(half4 *)(cu_sc + os + (q >> 1) * (1024 * 32) + 16 * 32 * (q & 1)) = act_quad<0>(accs[q >> 1][q & 1], a.scale5, *(const float4v *)(bl5 + 64 + 16 * (q >> 1)), false, none, false);
          }
        }
        L0_STEP_END();
        continue;
      }
      if (G5 >= 0 && G5 < 32 * nloc) {
        const int c = G5 >> 5, Y = G5 & 31, g0 = 2 * G5;
        const int lo = (2 * p) * PS + h * 16;      // output pixel p reads input columns 2p - 1 + dx = stored columns 2p + dx
        const uint32_t rows[3] = {lds_of(map_row(Or, nro, g0 - 1, 2 * Y - 1)) + lo, lds_of(Or + slot_of(nro, g0) * ROWB) + lo, lds_of(Or + slot_of(nro, g0 + 1) * ROWB) + lo};
        auto rd = [&](auto itc) {
          constexpr int item = decltype(itc)::value, tp = item >> 1, ks = item & 1, dy = tp / 3, dx = tp - dy * 3;
          lds_read128<dx * PS + ks * 32>(bf[item % PD], rows[dy]);
        };
        static_for<PD>([&](auto ic) { rd(ic); });
        float16v acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        static_for<18>([&](auto itc) {
          constexpr int item = decltype(itc)::value, e = item - (18 - PD);   // e >= 0: extra read number e follows this item
          lds_wait<((17 - item) < (PD - 1) ? (17 - item) : (PD - 1)) + (e > 0 ? e : 0)>();
          lds_touch(bf[item % PD]);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[item], bf[item % PD], acc, 0, 0, 0);
          if constexpr (item + PD < 18) rd(std::integral_constant<int, item + PD>{});
          else if constexpr (e < 2) lds_read128<PS + e * 32>(bf[item % PD], rows[1]);       // centre tap (dy 1, dx 1), k-step e
          else lds_read128<(e - 2) * 1024>(bf[item % PD], wsa);                               // shortcut weights, k-step e - 2
        });
        // t first (its accumulator dies before the shortcut's is born: the wave has 128 VGPRs), then the shortcut's two MFMAs and sc
        const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
        char *cu_t = (char *)a.y_t + n * (size_t)(32 * 32 * 64 * 2) + (Y * 32 * 64 + cb * 32) * 2;          // wave-uniform bases (SGPRs) ...
        char *cu_sc = (char *)a.y_sc + n * (size_t)(32 * 32 * 64 * 2) + (((2 * cb) << 10) + Y * 32) * 32;
        const uint32_t ot = (uint32_t)(p * 128 + h * 16), os = (uint32_t)(p * 32 + h * 16);                    // ... + lane offsets that do not change
        const float *bl5 = BL + 128 + 32 * cb + 4 * h;
        static_for<2>([&](auto qc) {
          constexpr int qq = decltype(qc)::value;
          const half4 none{};
          const half4 h0 = act_quad<2 * qq>(acc, a.scale5, *(const float4v *)(bl5 + 8 * (2 * qq)), false, none, true);
          const half4 h1 = act_quad<2 * qq + 1>(acc, a.scale5, *(const float4v *)(bl5 + 8 * (2 * qq + 1)), false, none, true);
          *(uint4v *)(cu_t + ot + 32 * qq) = pair16(h0, h1);
        });
        lds_wait<0>();
        static_for<PD>([&](auto ic) { lds_touch(bf[decltype(ic)::value]); });
        float16v accs;
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[i] = 0.f;
        accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[(18 - PD + 2) % PD], bf[(18 - PD) % PD], accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(bf[(18 - PD + 3) % PD], bf[(18 - PD + 1) % PD], accs, 0, 0, 0);
        static_for<2>([&](auto qc) {
          constexpr int qq = decltype(qc)::value;
          const half4 none{};
          const half4 s0 = act_quad<2 * qq>(accs, a.scale5, *(const float4v *)(bl5 + 64 + 8 * (2 * qq)), false, none, false);
          const half4 s1 = act_quad<2 * qq + 1>(accs, a.scale5, *(const float4v *)(bl5 + 64 + 8 * (2 * qq + 1)), false, none, false);
          // sc chunk-major, as the 64-channel chain reads it ([n][64 / 16][32 x 32][16] fp16; this lane: channels 8h .. 8h + 7 of chunk 2 cb + qq)
          *(uint4v *)(cu_sc + os + qq * (1024 * 32)) = pair16(s0, s1);
        });
      }
      L0_STEP_END();
    }
  }
#undef L0_STEP_END
}
template <bool F5, bool M16>
__global__ __launch_bounds__(1024) void layer0_stream_kernel(const Layer0Args a) { layer0_stream_body<F5, M16, false>(a); }
__global__ __launch_bounds__(1024) void layer0_stream_xs_kernel(const Layer0Args a) { layer0_stream_body<true, true, true>(a); }   // five stages, 16x16x32, xs hand-off
