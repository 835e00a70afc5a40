// mlt_layer1_kernel.inc -- layer1_stream_kernel: the three stride-1 convs of layer1 (64 channels at 32 x 32) as a streaming pipeline; part of mlt_kernels.hip.
// ---------------------------------------------------------------------------------------------
// Round 5.  chain_kernel<64> keeps a whole 128 KiB sample in LDS and streams the weights past it (216 KiB per sample through a ring:
// 28 % of its time in ring waits and barriers, `b0` through HBM because eight accumulators per wave leave no room for it).  Here, as in
// layer0_stream_kernel, the map flows and the WEIGHTS stay: one persistent 16-wave workgroup per CU walks the 32 rows of the map,
//     b0  = relu(bn2(conv2(t)) + sc)      (t, sc from layer0_stream_kernel's fifth stage: t NHWC, sc chunk-major)
//     u   = relu(bn1'(conv1'(b0)))
//     out = relu(bn2'(conv2'(u)) + b0)    -> HBM (NHWC or chunk-major) + fp32 GAP partial sums
// A 64 -> 64 conv has 72 A fragments (288 VGPRs): too many for a wave even per 32 output channels (36).  So every conv is FOUR waves: output
// channels 0-31 / 32-63 x the first / second half of the k order (taps 0-3 + half of tap 4 | the rest).  The second-half wave CONTINUES the
// first-half wave's accumulators, handed over through LDS as fp32 (4 KiB per 32 x 32 block, one step later): the summation order -- and with
// it every bit -- is chain_kernel's.  Twelve conv waves (18 A fragments = 72 VGPRs each, resident for the whole launch) and four loader waves (one
// 1 KiB piece of a t row and of an sc row each, register-staged, issued half a step group ahead).  The last conv activates, adds b0 and stores in
// its own waves and hands its fp32 values (after the ReLU) to 2 x 32 GAP lanes on two of the loader waves, which reproduce conv_epilogue's
// butterfly -- a balanced tree of commutative adds over chain_kernel's RANKED pixels -- one lane per channel, straight from LDS.
// One 32-pixel row per step and stage, one barrier per step; rings of 4 / 8 / 4 rows (34 pixels x 144 B) for t / b0 / u.
//
// Round 6, M16 = true (the default): the conv waves issue v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_32x32x16_f16.  One 16x16x32 MFMA gives, bit for
// bit, what two chained 32x32x16 MFMAs over the same 32 k values give (scripts/probes/mfma_shape_bits_probe.hip: 0 of 4,096,000 elements differ, alone
// and in chains of nine) -- so the summation order, and every logit, stays chain_kernel's -- while under the package's power cap the chip holds a 13 %
// higher clock on it: +11 % FLOP/s in a bare loop of this structure (weights in registers, one fragment read per 32 kFLOP;
// profiles/r06a_mfma_shape_probe.txt).  Per 32 input channels of a tap a wave now runs 2 cout blocks x 2 pixel halves = four MFMAs on two weight
// fragments (16 couts x 32 cin, gathered from the same packed weights) and two activation fragments (16 pixels x 32 cin: ONE ds_read_b128 per lane,
// channels 8 g .. 8 g + 7 of pixel l & 15): the same 18 + 18 fragments per row and the same 16 accumulator registers; a lane ends up with 4
// consecutive output channels of TWO pixels per block (no permlane pairing: 8-byte ring writes and stores).  M16 = false is round 5's form (A/B).
// ---------------------------------------------------------------------------------------------
#ifndef CFG_L1_PD
#define CFG_L1_PD 4
#endif
#ifndef CFG_L1_KO
#define CFG_L1_KO 0      // measurement only (results wrong): 1 the epilogue waves do nothing, 2 no accumulator hand-over (first halves do not store, second halves start from zero), 4 loaders idle
#endif
// XS (the 32x32x16 form only; layer1_stream_xs_kernel, behind layer0_stream_xs_kernel): `a.sc` holds xs -- the even pixels of the even rows of layer0's
// output, [n][32][32][32] fp16 -- instead of the projection shortcut, and the two loader waves that carry no GAP sums (14, 15: cout block cb = wave - 14)
// compute the shortcut row themselves: sc = bn(conv1x1 stride 2) is a K = 32 product, two chained 32x32x16 MFMAs from a zero accumulator on two A
// fragments that stay in registers (tap 9 of the packed stride-2 weights) and the row's two B fragments straight from HBM (lane (p, h), k step ks: channels
// 16 ks + 8 h .. + 7 of pixel p), then S5's epilogue expression and the 16-byte stores into the Sc slot that `commit` filled.  Same bits as S5's one
// 16x16x32 MFMA (scripts/probes/mfma_shape_bits_probe.hip); the conv waves, the slot timing and the rings do not change.  The sc row of 128 B per pixel
// neither leaves the front kernel nor comes back: 64 B per pixel do.
// xs rows in flight: four register slots of two fragments.  Slots 0 / 1 hold the rows of steps k0, k0 + 1 of a step group and are re-issued, right after
// their use, for steps k0 + 4, k0 + 5 (drained with the t rows at the group's end, three steps later); slots 2 / 3 are issued in the same two steps for
// steps k0 + 2, k0 + 3 of the SAME group (two steps ahead, counted waits) -- every load is issued in the first half of a group, as the t rows are.
template <bool M16, bool XS>
__device__ __forceinline__ void layer1_stream_body(const Layer1Args &a) {
  static_assert(!XS || !M16, "the xs hand-off exists for the 32x32x16 form");
  constexpr int PS = 144, RW = 34, ROWB = RW * PS;               // map rows: zero pixel, 32 pixels of 64 channels (+ 16 B), zero pixel
  constexpr int NRT = 4, NRB = 8, NRU = 4;                       // ring slots: t, b0 (also the last conv's residual), u
  constexpr int HB = 4096;                                       // one accumulator block in LDS: [quad 4][lane 64][16 B]
  constexpr int HEQ = 1104, HEH = 576, HE = 4 * HEQ;             // last conv -> GAP lanes: [quad 4][lane half 2][pixel 32][16 B], quads 1104 B and halves 576 B apart: the
                                                                 // 16-byte writes of a half-wave are contiguous AND the 32 four-byte reads of a GAP step hit 32 banks
  constexpr int PD = CFG_L1_PD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Tr = smem, *Br = Tr + NRT * ROWB, *Ur = Br + NRB * ROWB, *Z = Ur + NRU * ROWB;
  char *Sc = Z + ROWB;                                           // sc rows, chunk-major as in HBM: [slot 2][chunk 4][pixel 32][32 B]
  char *Hd = Sc + 2 * 4096;                                      // accumulator hand-over: [link 4][cout block 2][slot 2][HB]; links: conv 0/1/2 first -> second half, conv 2 -> epilogue
  char *He = Hd + 3 * 2 * 2 * HB;                                // [cout block 2][slot 2][HE]
  float *BL = (float *)(He + 2 * 2 * HE);                        // biases [conv 3][64]; XS: + the shortcut's [64]
  constexpr int ZERO_BYTES = (NRT + NRB + NRU + 1) * ROWB + 2 * 4096;
  static_assert(ZERO_BYTES % 16 == 0 && MLT_L1_LDS_BYTES == ZERO_BYTES + 3 * 2 * 2 * HB + 2 * 2 * HE + 3 * 64 * 4 && MLT_L1X_LDS_BYTES == MLT_L1_LDS_BYTES + 64 * 4, "LDS layout");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = lane & 31, h = lane >> 5;
  if ((int)blockIdx.x >= a.n) return;
  const int nloc = (a.n - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int rows_total = 32 * nloc, ksteps = rows_total + 11;
  for (int o = tid * 16; o < ZERO_BYTES; o += 1024 * 16) *(uint4v *)(smem + o) = uint4v{0u, 0u, 0u, 0u};
  if (tid < 192) BL[tid] = a.bias[tid >> 6][tid & 63];
  if (XS && tid >= 192 && tid < 256) BL[tid] = a.bias_sc[tid - 192];
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  auto lds_of = [&](const char *q) -> uint32_t { return lds0 + (uint32_t)(q - smem); };
  auto row_of = [&](char *ring, int mask, int g, int r) -> const char * { return (r >= 0 && r < 32) ? ring + (g & mask) * ROWB : Z; };
#define L1_STEP_END() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

  if (wave < 12) {
    // ================= conv waves: pair -> (conv, half of the k order); SIMDs 0 / 1 host c2 first, c3 second, c4 first; SIMDs 2 / 3 the others =================
    const int pair = wave >> 1, cb = wave & 1;
    const int cv = pair < 2 ? 0 : pair < 4 ? 1 : 2;
    const bool second = pair == 1 || pair == 2 || pair == 5;
    const int lag = cv == 0 ? (second ? 3 : 2) : cv == 1 ? (second ? 6 : 5) : (second ? 9 : 8);
    char *in_ring = cv == 0 ? Tr : cv == 1 ? Br : Ur;
    const int in_mask = cv == 1 ? NRB - 1 : NRT - 1;
    half8 wf[18];
    const int p16 = lane & 15, g4 = lane >> 4;   // M16: pixel (of a 16-pixel half) / channel group of 8 (B operand), cout (of a 16-cout block) / k group (A operand)
    if constexpr (!M16) {
      const char *w = (const char *)a.w[cv] + (((second ? 18 : 0) * 2 + cb) * 1024) + lane * 16;
#pragma unroll
      for (int i = 0; i < 18; ++i) wf[i] = *(const half8 *)(w + i * 2048);
    } else {
      // fragment 2 s + c: 32-channel k step s of this half of the k order, couts 16 c .. 16 c + 15 of the wave's 32: lane (i, g) holds
      // W[cout 16 c + i][k 8 g .. 8 g + 7] = the 32x32x16 packing's fragment of k16 step 2 s + (g >> 1), lane (g & 1) * 32 + 16 c + i
#pragma unroll
      for (int i = 0; i < 18; ++i) {
        const int item = (second ? 18 : 0) + (i & ~1) + (g4 >> 1), lsrc = (g4 & 1) * 32 + 16 * (i & 1) + p16;
        wf[i] = *(const half8 *)((const char *)a.w[cv] + (size_t)(((item * 2 + cb) * 64 + lsrc) * 16));
      }
    }
#pragma unroll
    for (int i = 0; i < 18; ++i) asm volatile("" ::"v"(wf[i]));
    char *hand = Hd + ((cv * 2 + cb) * 2) * HB;                  // link cv (first -> second half)
    char *hand_e = He + (cb * 2) * HE;                           // last conv -> GAP wave
    const float scale = a.scale[cv];
    L1_STEP_END();
    for (int k = 0; k < ksteps; ++k) {
      const int g = k - lag;
      if (g >= 0 && g < rows_total) {
        const int r = g & 31;
        const int lo = M16 ? p16 * PS + g4 * 16 : p * PS + h * 16;
        const uint32_t rows[3] = {lds_of(row_of(in_ring, in_mask, g - 1, r - 1)) + lo, lds_of(in_ring + (g & in_mask) * ROWB) + lo, lds_of(row_of(in_ring, in_mask, g + 1, r + 1)) + lo};
        half8 bf[PD];
        if constexpr (M16) {
          // ---- 16x16x32: item j = 2 s + half (s: 32-channel k step, half: pixels 0-15 / 16-31 of the row); two MFMAs (cout blocks) per item ----
          float4v acc[2][2];   // [cout block c][pixel half]
          auto run = [&](auto secc) {
            constexpr int S0 = decltype(secc)::value ? 9 : 0;
            auto rd = [&](auto itc) {
              constexpr int item = decltype(itc)::value, S = S0 + (item >> 1), hf = item & 1, tap = S >> 1, kh = S & 1, dy = tap / 3, dx = tap - dy * 3;
              lds_read128<(dx + 16 * hf) * PS + kh * 64>(bf[item % PD], rows[dy]);
            };
            static_for<PD>([&](auto ic) { rd(ic); });
            static_for<18>([&](auto itc) {
              constexpr int item = decltype(itc)::value, s = item >> 1, hf = item & 1;
              lds_wait<((17 - item) < (PD - 1) ? (17 - item) : (PD - 1))>();
              lds_touch(bf[item % PD]);
              acc[0][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * s], bf[item % PD], acc[0][hf], 0, 0, 0);
              acc[1][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[2 * s + 1], bf[item % PD], acc[1][hf], 0, 0, 0);
              if constexpr (item + PD < 18) rd(std::integral_constant<int, item + PD>{});
            });
          };
          if (!second) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q >> 1][q & 1] = float4v{0.f, 0.f, 0.f, 0.f};
            run(std::false_type{});
            char *hw = hand + (k & 1) * HB + lane * 16;
            if (CFG_L1_KO & 2) { asm volatile("" ::"v"(acc[0][0]), "v"(acc[0][1]), "v"(acc[1][0]), "v"(acc[1][1])); }
            else
#pragma unroll
            for (int q = 0; q < 4; ++q) *(float4v *)(hw + q * 1024) = acc[q >> 1][q & 1];
          } else {
            const char *hr = hand + ((k - 1) & 1) * HB + lane * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q >> 1][q & 1] = (CFG_L1_KO & 2) ? float4v{0.f, 0.f, 0.f, 0.f} : *(const float4v *)(hr + q * 1024);
            run(std::true_type{});
            // epilogues: act_quad's expressions on the four values a lane holds per block -- couts cb * 32 + 16 c + 4 g .. + 3 of pixel 16 half + (l & 15)
            if (cv == 2) {
              const int c_ = g >> 5;
              const size_t n = (size_t)blockIdx.x + (size_t)c_ * gridDim.x;
              char *cu_y = (char *)a.y + n * (size_t)(32 * 32 * 64 * 2);
              char *hwe = hand_e + (k & 1) * HE;
              static_for<4>([&](auto qc) {
                constexpr int c = decltype(qc)::value >> 1, hf = decltype(qc)::value & 1;
                const int pix = 16 * hf + p16;
                const half4 res = *(const half4 *)(Br + (g & (NRB - 1)) * ROWB + (pix + 1) * PS + cb * 64 + c * 32 + 8 * g4);   // residual: this row of b0
                float v[4];
                const half4 o4 = act_quad<0>(acc[c][hf], scale, *(const float4v *)(BL + 2 * 64 + cb * 32 + 16 * c + 4 * g4), true, res, true, v);
                const uint32_t oy = a.y_c16 ? (uint32_t)(((((2 * cb + c) << 10) + r * 32 + pix) * 16 + 4 * g4) * 2)       // chunk-major [n][4][1024][16]
                                            : (uint32_t)((((r * 32 + pix) * 64) + cb * 32 + 16 * c + 4 * g4) * 2);         // NHWC
                *(half4 *)(cu_y + oy) = o4;
                // the GAP lanes' image: channel 8 q + 4 hh + e of pixel pix at q * HEQ + hh * HEH + pix * 16 + 4 e (q = 2 c + (g >> 1), hh = g & 1)
                *(float4v *)(hwe + (2 * c + (g4 >> 1)) * HEQ + (g4 & 1) * HEH + pix * 16) = float4v{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
              });
            } else {
              char *drow = (cv == 0 ? Br + (g & (NRB - 1)) * ROWB : Ur + (g & (NRU - 1)) * ROWB);
              static_for<4>([&](auto qc) {
                constexpr int c = decltype(qc)::value >> 1, hf = decltype(qc)::value & 1;
                const int pix = 16 * hf + p16;
                half4 res{};
                if (cv == 0) res = *(const half4 *)(Sc + ((g & 1) * 4 + 2 * cb + c) * 1024 + pix * 32 + 8 * g4);   // sc row g, chunk 2 cb + c, this lane's 4 channels
                const half4 o4 = act_quad<0>(acc[c][hf], scale, *(const float4v *)(BL + cv * 64 + cb * 32 + 16 * c + 4 * g4), cv == 0, res, true);
                *(half4 *)(drow + (pix + 1) * PS + cb * 64 + c * 32 + 8 * g4) = o4;
              });
            }
          }
        } else {
        float16v acc;
        auto run = [&](auto secc) {
          constexpr int I0 = decltype(secc)::value ? 18 : 0;
          auto rd = [&](auto itc) {
            constexpr int item = decltype(itc)::value, it = I0 + item, tap = it >> 2, ks = it & 3, dy = tap / 3, dx = tap - dy * 3;
            lds_read128<dx * PS + ks * 32>(bf[item % PD], rows[dy]);
          };
          static_for<PD>([&](auto ic) { rd(ic); });
          static_for<18>([&](auto itc) {
            constexpr int item = decltype(itc)::value;
            lds_wait<((17 - item) < (PD - 1) ? (17 - item) : (PD - 1))>();
            lds_touch(bf[item % PD]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[item], bf[item % PD], acc, 0, 0, 0);
            if constexpr (item + PD < 18) rd(std::integral_constant<int, item + PD>{});
          });
        };
        if (!second) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = 0.f;
          run(std::false_type{});
          char *hw = hand + (k & 1) * HB + lane * 16;
          if (CFG_L1_KO & 2) asm volatile("" ::"v"(acc));
          else
#pragma unroll
          for (int q = 0; q < 4; ++q) *(float4v *)(hw + q * 1024) = float4v{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        } else {
          const char *hr = hand + ((k - 1) & 1) * HB + lane * 16;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4v v = (CFG_L1_KO & 2) ? float4v{0.f, 0.f, 0.f, 0.f} : *(const float4v *)(hr + q * 1024);
            acc[4 * q] = v[0]; acc[4 * q + 1] = v[1]; acc[4 * q + 2] = v[2]; acc[4 * q + 3] = v[3];
          }
          run(std::true_type{});
          if (cv == 2) {
            // the last conv: activation + residual + HBM store here (conv_epilogue's expressions for NSPLIT == 1: act_quad with the fp32 values
            // before the ReLU kept for the GAP); the GAP butterfly itself -- a long chain of cross-lane steps -- belongs to the epilogue waves, which
            // get the fp32 values (after the ReLU) through LDS: with the whole epilogue there, two waves' latency chain was the step (knock-out: 0.77 -> 1.00 ms)
            const float *bl = BL + 2 * 64 + cb * 32 + 4 * h;
            const char *rs = Br + (g & (NRB - 1)) * ROWB + (p + 1) * PS + cb * 64 + 16 * h;   // residual: this row of b0
            const int c = g >> 5;
            const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
            char *cu_y = (char *)a.y + n * (size_t)(32 * 32 * 64 * 2);
            float v[16];
            static_for<2>([&](auto qc) {
              constexpr int qq = decltype(qc)::value;
              half4 ra, rb;
              unpair16(*(const uint4v *)(rs + 32 * qq), ra, rb);
              const half4 h0 = act_quad<2 * qq>(acc, scale, *(const float4v *)(bl + 8 * (2 * qq)), true, ra, true, &v[4 * (2 * qq)]);
              const half4 h1 = act_quad<2 * qq + 1>(acc, scale, *(const float4v *)(bl + 8 * (2 * qq + 1)), true, rb, true, &v[4 * (2 * qq + 1)]);
              const uint32_t oy = a.y_c16 ? (uint32_t)(((((2 * cb + qq) << 10) + r * 32 + p) * 16 + 8 * h) * 2)    // chunk-major [n][4][1024][16]
                                          : (uint32_t)((((r * 32 + p) * 64) + cb * 32 + 8 * h + 16 * qq) * 2);      // NHWC
              *(uint4v *)(cu_y + oy) = pair16(h0, h1);
            });
            char *hw = hand_e + (k & 1) * HE + h * HEH + p * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(float4v *)(hw + q * HEQ) = float4v{fmaxf(v[4 * q], 0.f), fmaxf(v[4 * q + 1], 0.f), fmaxf(v[4 * q + 2], 0.f), fmaxf(v[4 * q + 3], 0.f)};
          } else {
            const float *bl = BL + cv * 64 + cb * 32 + 4 * h;
            const char *rs = Sc + ((g & 1) * 4 + 2 * cb) * 1024 + p * 32 + 16 * h;   // conv 0: sc row g, chunks 2 cb / 2 cb + 1, this lane's 8 channels
            char *dst = (cv == 0 ? Br + (g & (NRB - 1)) * ROWB : Ur + (g & (NRU - 1)) * ROWB) + (p + 1) * PS + cb * 64 + 16 * h;
            static_for<2>([&](auto qc) {
              constexpr int qq = decltype(qc)::value;
              half4 ra{}, rb{};
              if (cv == 0) unpair16(*(const uint4v *)(rs + qq * 1024), ra, rb);
              const half4 h0 = act_quad<2 * qq>(acc, scale, *(const float4v *)(bl + 8 * (2 * qq)), cv == 0, ra, true);
              const half4 h1 = act_quad<2 * qq + 1>(acc, scale, *(const float4v *)(bl + 8 * (2 * qq + 1)), cv == 0, rb, true);
              *(uint4v *)(dst + 32 * qq) = pair16(h0, h1);
            });
          }
        }
        }
      }
      L1_STEP_END();
    }
  } else {
    // ================= waves 12-15: each the loader of one of a row's four 1 KiB pieces (t row k and sc row k - 2 at step k); waves 12, 13 also the GAP sums of 32 output channels =================
    // (issued half a step group ahead and converted a group later, as layer0_stream_kernel's raw rows: with two steps per group the group's end waited for HBM)
    // GAP: conv_epilogue's butterfly over the 32 lanes of an MFMA block is a balanced tree of fp32 adds whose leaves are chain_kernel's RANKED pixels
    // (lane p holds pixel pr(p)); every add is "kept + received", i.e. commutative, so the tree over adjacent leaves reproduces it bit for bit --
    // computed here by ONE lane per channel straight from LDS (32 reads at compile-time offsets, 31 adds, no cross-lane step: with the butterfly's
    // sixteen ds_bpermute in five dependent levels on a busy LDS, two waves' latency chain was the step).
    const int li = wave - 12;
    constexpr int RD = 4, NP = 1;
    uint4v tc[RD][NP], sc_[RD][NP], tn[RD][NP], sn[RD][NP];
    auto issue = [&](uint4v (&tv)[NP], uint4v (&sv)[NP], int k) {  // (unconditional, rows behind the last CU clamped: counted waits)
      int gt = k, gs = k - 2;
      gt = gt < 0 ? 0 : gt < rows_total ? gt : rows_total - 1;
      gs = gs < 0 ? 0 : gs < rows_total ? gs : rows_total - 1;
      const size_t nt = (size_t)blockIdx.x + (size_t)(gt >> 5) * gridDim.x, ns = (size_t)blockIdx.x + (size_t)(gs >> 5) * gridDim.x;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int ch = NP * li + i;
        tv[i] = *(const uint4v *)((const char *)a.t + (nt * 1024 + (size_t)(gt & 31) * 32) * 128 + ch * 1024 + lane * 16);
        if constexpr (!XS) sv[i] = *(const uint4v *)((const char *)a.sc + (((ns * 4 + ch) << 10) + (size_t)(gs & 31) * 32) * 32 + lane * 16);
      }
    };
    // XS, waves 14 / 15: the two B fragments of xs row k - 2 (unconditional and clamped, as above), and the shortcut row from them
    const int cbx = li & 1;
    half8 xa[2];
    uint4v xr[RD][2];
    auto issue_x = [&](uint4v (&xv)[2], int k) {
      int gs = k - 2;
      gs = gs < 0 ? 0 : gs < rows_total ? gs : rows_total - 1;
      const size_t ns = (size_t)blockIdx.x + (size_t)(gs >> 5) * gridDim.x;
      const char *src = (const char *)a.sc + ((ns * 1024 + (size_t)(gs & 31) * 32 + p) * 32 + 8 * h) * 2;
      xv[0] = *(const uint4v *)src;
      xv[1] = *(const uint4v *)(src + 32);
    };
    auto sc_row = [&](const uint4v (&xv)[2], int k) {
      const int gs = k - 2;
      if (gs >= 0 && gs < rows_total) {
        float16v accs;
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[i] = 0.f;
        accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[0], *(const half8 *)&xv[0], accs, 0, 0, 0);
        accs = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[1], *(const half8 *)&xv[1], accs, 0, 0, 0);
        const float *bl = BL + 3 * 64 + cbx * 32 + 4 * h;
        char *dst = Sc + ((gs & 1) * 4 + 2 * cbx) * 1024 + p * 32 + 16 * h;   // chunks 2 cb / 2 cb + 1, this lane's 8 channels
        static_for<2>([&](auto qc) {
          constexpr int qq = decltype(qc)::value;
          const half4 none{};
          const half4 s0 = act_quad<2 * qq>(accs, a.scale_sc, *(const float4v *)(bl + 8 * (2 * qq)), false, none, false);
          const half4 s1 = act_quad<2 * qq + 1>(accs, a.scale_sc, *(const float4v *)(bl + 8 * (2 * qq + 1)), false, none, false);
          *(uint4v *)(dst + qq * 1024) = pair16(s0, s1);
        });
      }
    };
    auto commit = [&](const uint4v (&tv)[NP], const uint4v (&sv)[NP], int k) {
      const int gt = k, gs = k - 2;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int ch = NP * li + i;
        if (gt >= 0 && gt < rows_total) *(uint4v *)(Tr + (gt & (NRT - 1)) * ROWB + (8 * ch + (lane >> 3) + 1) * PS + (lane & 7) * 16) = tv[i];
        if (!XS && gs >= 0 && gs < rows_total) *(uint4v *)(Sc + ((gs & 1) * 4 + ch) * 1024 + lane * 16) = sv[i];
      }
    };
    const int cb = li & 1, ch = lane & 31;
    const int hh = (ch >> 2) & 1;                                   // channel 8 q + 4 h + e lives in accumulator register 4 q + e of lane half h
    const char *gbase = He + (cb * 2) * HE + (ch >> 3) * HEQ + hh * HEH + (ch & 3) * 4;
    auto gap_row = [&](int k) {
      const int g = k - 10;
      if (li < 2 && lane < 32 && g >= 0 && g < rows_total && !(CFG_L1_KO & 1)) {
        const int c = g >> 5, r = g & 31;
        const size_t n = (size_t)blockIdx.x + (size_t)c * gridDim.x;
        const char *src = gbase + ((k - 1) & 1) * HE;
        float x[32];
        static_for<32>([&](auto tc_) {
          constexpr int t = decltype(tc_)::value;
          constexpr int pr = t < 4 ? t : t < 12 ? t + 12 : t < 16 ? t - 8 : t < 20 ? t + 8 : t < 28 ? t - 12 : t;   // chain_kernel's lane -> pixel ranking
          x[t] = *(const float *)(src + pr * 16);
        });
#pragma unroll
        for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
          for (int i = 0; i < w; ++i) x[i] = x[2 * i] + x[2 * i + 1];
        a.gap[(n * a.gap_slots + r) * 64 + cb * 32 + ch] = x[0];
      }
    };
    // XS: the loop exists twice, once per role (waves 12 / 13: t + GAP, waves 14 / 15: t + shortcut) -- a wave-uniform branch around the xs loads inside
    // ONE loop makes the compiler's wait for a row count the younger loads of the path that issued none, and the counted waits become drains
    auto loader = [&](auto xsc) {
      constexpr bool X = decltype(xsc)::value;   // this wave computes the shortcut rows
#pragma unroll
      for (int d = 0; d < RD; ++d) issue(tc[d], sc_[d], d);
      if constexpr (X) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) xa[ks] = *(const half8 *)((const char *)a.w_sc + ((18 + ks) * 2 + cbx) * 1024 + lane * 16);   // tap 9 of the packed stride-2 weights
        asm volatile("" ::"v"(xa[0]), "v"(xa[1]));
        issue_x(xr[0], 0);
        issue_x(xr[1], 1);
      }
      L1_STEP_END();
      // (X: whole step groups only, with no way round a slot -- a path on which slot 1 is skipped and slot 2 runs exists for the compiler, and on it the
      // rows of slots 2 / 3 are the youngest loads: their waits came out as drains.  ksteps = 32 nloc + 11 leaves three steps, which touch no t / sc row.)
      int k0 = 0;
      for (; X ? k0 + RD <= ksteps : k0 < ksteps; k0 += RD) {
        static_for<RD>([&](auto slc) {
          constexpr int sl = decltype(slc)::value;
          const int k = k0 + sl;
          if constexpr (!X) { if (k >= ksteps) return; }
          if (!(CFG_L1_KO & 4)) commit(tc[sl], sc_[sl], k);
          if constexpr (sl < RD / 2 && !(CFG_L1_KO & 4)) {
            issue(tn[2 * sl], sn[2 * sl], k0 + RD + 2 * sl);
            issue(tn[2 * sl + 1], sn[2 * sl + 1], k0 + RD + 2 * sl + 1);
          }
          if constexpr (X && !(CFG_L1_KO & 4)) {
            sc_row(xr[sl], k);
            if constexpr (sl < RD / 2) {
              issue_x(xr[RD / 2 + sl], k0 + RD / 2 + sl);   // (the nearer row first: its wait leaves the other one in flight)
              issue_x(xr[sl], k0 + RD + sl);
            }
          }
          if constexpr (!X) gap_row(k);
          L1_STEP_END();
        });
#pragma unroll
        for (int d = 0; d < RD; ++d)
#pragma unroll
          for (int i = 0; i < NP; ++i) { tc[d][i] = tn[d][i]; sc_[d][i] = sn[d][i]; }
      }
      if constexpr (X)
        for (; k0 < ksteps; ++k0) L1_STEP_END();   // k0 >= rows_total + 8: behind the last t row (k) and the last sc row (k - 2)
    };
    if (XS && li >= 2) loader(std::true_type{});
    else loader(std::false_type{});
  }
#undef L1_STEP_END
}
template <bool M16>
__global__ __launch_bounds__(1024) void layer1_stream_kernel(const Layer1Args a) { layer1_stream_body<M16, false>(a); }
__global__ __launch_bounds__(1024) void layer1_stream_xs_kernel(const Layer1Args a) { layer1_stream_body<false, true>(a); }   // 32x32x16, xs hand-off
