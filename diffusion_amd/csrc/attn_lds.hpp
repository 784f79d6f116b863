// LDS tile images and MFMA fragment helpers shared by the attention kernels (attention.hip, attention_wide.hip): the
// [rows][64 bf16] image with XOR-swizzled 128-B rows (swz_key, described in attention.hip), its row and transposed reads,
// the LDS-DMA fill and the accumulator map of v_mfma_f32_32x32x16_bf16.
#pragma once
#include "common.hpp"

namespace {

constexpr int TR_LD = 128;
DEVINL int swz_key(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
DEVINL int tr_off(int row, int bytecol) { return row * TR_LD + (bytecol ^ (swz_key(row) << 4)); }

DEVINL int swz128(int row, int chunk) { return row * 128 + ((chunk ^ swz_key(row)) << 4); }

// A operand of the 32x32x16 MFMA for (rows = columns col0..col0+31 of a transposed-read image, k = 16 image rows
// starting at row0) in the accumulator-as-operand k order: element j <-> image row row0 + 8*(j>>2) + 4*(lane>>5) + (j&3).
// Issued in two steps because every loop here also fills LDS by DMA: the two transposed reads go through the asm form
// (common.hpp: against the intrinsic the compiler waits for every pending DMA), the caller waits with lds_wait_for<>
// and then joins the halves.
DEVINL void tr_frag_issue(unsigned img_off, int row0, int col0, int lane, short4v& t0, short4v& t1) {
  const int gg = lane >> 4, dgrp = gg & 1, hh = gg >> 1, qq = (lane >> 2) & 3, pp = lane & 3;
  const int row = row0 + 4 * hh + qq, bc = (col0 + 16 * dgrp + 4 * pp) * 2;
  const unsigned a = img_off + tr_off(row, bc);
  t0 = lds_tr16_b64_asm(a);
  // row + 8 flips bit 3 of the row = bit 1 of swz_key = byte bit 5 of the column (image offsets are multiples of 128 B)
  t1 = lds_tr16_b64_asm((a ^ 32u) + 8 * TR_LD);
}
DEVINL bf16x8 tr_frag_join(short4v t0, short4v t1) {
  typedef __attribute__((ext_vector_type(8))) short short8v;
  short8v v = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

DEVINL bf16x8 pack8(const f32x16& x, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f2bf(x[8 * s + j]);
  return r;
}

// LDS-DMA (global_load_lds): 64 lanes x 16 B land lane-linearly at a wave-uniform LDS address (see attention.hip)
DEVINL void dma16(const void* g, char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

DEVINL int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

}  // namespace
