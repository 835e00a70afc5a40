// mlt_picture_kernels.inc -- device-resident pictures (include/mltcnn.h: mlt_predict_at): CUs named by the position of their top-left luma sample are gathered
// out of two pitched planes into the dense [c][S][S] staging planes every batch entry point feeds the network from.  Included by mlt_kernels.hip.
//
// HBM-bound copy.  A work item = 8 consecutive pixels of one row of one plane of one CU = ONE 16-byte store (the staging planes are 256-byte aligned and a row of
// S >= 16 pixels is a whole number of items, so every store is aligned); items are numbered plane-major, then CU, row, 8-pixel segment -- consecutive lanes write
// consecutive 16 bytes and read consecutive 16 bytes of a picture row -- and a flat grid-stride loop walks them, so a 16 x 16 CU (64 items) costs one wave, not a
// workgroup.  Three source paths, chosen per item from the BYTE address of its first pixel (with an odd pitch the misalignment changes from row to row):
//   aligned     the 8 pixels start on a 16-byte boundary: one 16-byte load
//   funnel      they do not: the two aligned 16-byte windows that hold them, shifted together by the byte offset (2, 4, ... 14)
//   element     eight 2-byte loads; needs only the 2-byte alignment of a Pel
// Correctness never rests on the hardware tolerating a misaligned vector access: every 16-byte load above is 16-byte aligned.
//
// NO LOAD TOUCHES A BYTE OUTSIDE THE PICTURE'S EXTENT.  The item's own 16 bytes lie inside it (the host checks every position against width and height before
// anything is enqueued).  The funnel path's two windows [lo, lo + 16) and [lo + 16, lo + 32), lo = address & ~15, each hold at least one of the item's bytes (its
// first byte is in the first, and with a non-zero offset its last byte is in the second), and a 16-byte window that is aligned and holds one byte of an extent
// that STARTS AND ENDS on 16-byte boundaries lies wholly inside that extent.  The host sets vec_org / vec_pred only for such extents:
//   library-owned pictures  hipMalloc'ed base, pitch a multiple of 8 elements, height x pitch x 2 bytes allocated: both ends aligned, always
//   wrapped pictures        only when the caller's base and base + ((height - 1) x stride + width) x 2 are both multiples of 16
// Every other plane takes the element path for all of its items.

typedef uint32_t pic_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ pic_u32x4 picture_fetch8(const int16_t *p, bool vec) {
  const uintptr_t addr = (uintptr_t)p;
  pic_u32x4 v;
  if (!vec) {   // element path
    const uint16_t *e = (const uint16_t *)p;
    v.x = e[0] | ((uint32_t)e[1] << 16); v.y = e[2] | ((uint32_t)e[3] << 16);
    v.z = e[4] | ((uint32_t)e[5] << 16); v.w = e[6] | ((uint32_t)e[7] << 16);
    return v;
  }
  const unsigned off = (unsigned)(addr & 15);   // even: Pels are 2-byte aligned
  const pic_u32x4 *lo = (const pic_u32x4 *)(addr - off);
  if (off == 0) return lo[0];   // aligned path
  // funnel path: bytes off .. off + 15 of the 32 bytes a, b
  const pic_u32x4 a = lo[0], b = lo[1];
  uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y, w6 = b.z, w7 = b.w;
  if (off & 8) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; w5 = w7; }   // whole dwords first (w6, w7 are not read again after a shift by two) ...
  if (off & 4) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
  if (off & 2) {                                                            // ... then the odd Pel: v_alignbyte_b32 takes (high, low, byte shift)
    w0 = __builtin_amdgcn_alignbyte(w1, w0, 2); w1 = __builtin_amdgcn_alignbyte(w2, w1, 2);
    w2 = __builtin_amdgcn_alignbyte(w3, w2, 2); w3 = __builtin_amdgcn_alignbyte(w4, w3, 2);
  }
  v.x = w0; v.y = w1; v.z = w2; v.w = w3;
  return v;
}

__global__ __launch_bounds__(256) void picture_gather_kernel(const PictureGatherArgs a) {
  const int seg_l = a.s_l - 3;                                  // 8-pixel segments per row = S / 8
  const size_t per_plane = (size_t)a.c << (2 * a.s_l - 3);      // items of one plane
  const size_t total = 2 * per_plane, step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const bool is_pred = i >= per_plane;
    const size_t j = is_pred ? i - per_plane : i;
    const int seg = (int)(j & ((1u << seg_l) - 1)), row = (int)((j >> seg_l) & ((1u << a.s_l) - 1)), cu = (int)(j >> (seg_l + a.s_l));
    const int x = a.xy[2 * cu], y = a.xy[2 * cu + 1];
    const int16_t *src = (is_pred ? a.pred : a.org) + (size_t)(y + row) * (size_t)(is_pred ? a.pred_pitch : a.org_pitch) + x + 8 * seg;
    const pic_u32x4 v = picture_fetch8(src, is_pred ? a.vec_pred != 0 : a.vec_org != 0);
    *(pic_u32x4 *)((is_pred ? a.g_pred : a.g_org) + 8 * j) = v;   // dense [c][S][S]: item j of the plane starts at element 8 j
  }
}

// picture_gather_kernel for CUs of SEVERAL picture pairs in one list (mlt_predict_trees): CU cu belongs to entry pic[cu] of a per-call table, which holds what
// the one-pair launch takes as arguments -- the two plane bases, pitches and alignment classes -- and the entry's poc / qp.  The alignment class is therefore a
// property of the ITEM, and the argument above holds per entry: the host validates every entry's geometry (all entries of a call share width and height, and the
// positions are complete CUs of that geometry), and sets an entry's vec flags from that entry's own extents.  The first item of a CU also writes the CU's poc / qp
// into the staging set, so a chunk that cuts through several pictures needs no fill of its own.
__global__ __launch_bounds__(256) void picture_gather_multi_kernel(const PictureGatherMultiArgs a) {
  const int seg_l = a.s_l - 3;
  const size_t per_plane = (size_t)a.c << (2 * a.s_l - 3);
  const size_t total = 2 * per_plane, step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const bool is_pred = i >= per_plane;
    const size_t j = is_pred ? i - per_plane : i;
    const int seg = (int)(j & ((1u << seg_l) - 1)), row = (int)((j >> seg_l) & ((1u << a.s_l) - 1)), cu = (int)(j >> (seg_l + a.s_l));
    const int p = a.pic[cu];
    if ((unsigned)p >= (unsigned)a.n_entries) continue;   // (the expand kernel writes indices below n_pictures only: never taken)
    const TreesEntry &e = a.entries[p];
    const int x = a.xy[2 * cu], y = a.xy[2 * cu + 1];
    const int16_t *src = (is_pred ? e.pred : e.org) + (size_t)(y + row) * (size_t)(is_pred ? e.pred_pitch : e.org_pitch) + x + 8 * seg;
    const pic_u32x4 v = picture_fetch8(src, is_pred ? e.vec_pred != 0 : e.vec_org != 0);
    *(pic_u32x4 *)((is_pred ? a.g_pred : a.g_org) + 8 * j) = v;
    if (!is_pred && seg == 0 && row == 0) { a.g_poc[cu] = e.poc; a.g_qp[cu] = e.qp; }
  }
}
