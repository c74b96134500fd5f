// C entry points around gpmp2_amd/csrc/rec_pieces.h for the CPU tests (tests/test_rec_pieces_cpu.py): the 16-byte pieces
// in which k_linearize_arm stores a chunk's records, built by the host compiler alone.  Nothing else lives here.
#include "rec_pieces.h"

extern "C" {

int shim_rec_npieces(int RECL) { return g2::rec_npieces(RECL); }

int shim_rec_live_points(int P, int p_lo) { return g2::rec_live_points(P, p_lo); }

int shim_rec_piece_count(int live, int RECL) { return g2::rec_piece_count(live, RECL); }

int shim_rec_lds_stride(int RECL) { return g2::rec_lds_stride(RECL); }

// out: point, pair, padded, src; returns dst
long shim_rec_piece(int e, int RECL, int RECS, int* out) {
  const g2::RecPiece pc = g2::rec_piece(e, RECL, RECS);
  out[0] = pc.point;
  out[1] = pc.pair;
  out[2] = pc.padded ? 1 : 0;
  out[3] = pc.src;
  return pc.dst;
}

}  // extern "C"
