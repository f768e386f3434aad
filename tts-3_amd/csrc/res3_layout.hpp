// LDS row layouts of the whole-block kernel's staged B operands (resblock_block.hpp).  Plain
// constexpr code with no device dependencies: tests_native/res3_layout_check.cpp includes it on
// the host and checks the bank behaviour of every access the kernel makes.
//
// A staged row is one time column of one 16-channel group: NP pieces of 32 bytes, each two 16-byte
// units (channel positions 0..7 and 8..15).  Logical unit lu = half + 2 piece.
//   padded   (SWZ = false): pitch 32 NP + 16, unit lu at byte 16 lu.  The pad makes the pitch
//            4 x odd dwords, which alone keeps ds_read_b128 / ds_write_b128 conflict-free.
//   swizzled (SWZ = true, NP = 2): pitch 64, no pad; unit lu of row r sits at physical unit
//            lu ^ ((r >> 2) & 3).  Four rows cover the 64 banks, so rows r and r + 4 j share
//            banks; a ds_read_b128 lane group holds, per row residue mod 4, the row quads
//            j0 + {0, 3, 5, 6} or j0 + {1, 2, 4, 7}, which are distinct mod 4: the XOR sends them to
//            four different units and every group touches 64 distinct banks at any row offset.
//            The 8-lane groups of a ds_write_b128 (and the 16-lane groups of the prologue's
//            ds_write_b64) see 32 banks = 2 rows, so 4 of their 8 rows share a parity; those span at
//            most 3 row quads: 2-way at worst, which a 16-byte store's own issue time covers.
#pragma once

namespace tts {

template <int NP, bool SWZ>
struct Res3Rows {
  static_assert(!SWZ || NP == 2, "the swizzle permutes the 4 units of a two-piece row");
  static constexpr int UNITS = 2 * NP;
  static constexpr int PITCH = SWZ ? 32 * NP : 32 * NP + 16;
  // (row, logical unit) -> physical unit; row is the row index in the whole staged region
  static constexpr int unit(int row, int lu) { return SWZ ? (lu ^ ((row >> 2) & 3)) : lu; }
  // byte offset of logical unit lu of row `row` from the region's start
  static constexpr int off(int row, int lu) { return row * PITCH + 16 * unit(row, lu); }
  // from the offset of unit lu (piece 0: lu < 2) to the same half of piece q: off(row, lu + 2 q).
  // Rows r and r + 16 j have the same unit map, so off(row + 16 j, lu) = off(row, lu) + 16 j PITCH
  static constexpr int piece(int off0, int q) { return SWZ ? (off0 ^ (32 * q)) : off0 + 32 * q; }
  static constexpr bool SWIZZLED = SWZ;
};

}  // namespace tts
