// rec_pieces.h -- the 16-byte pieces in which the four wavefronts of k_linearize_arm store the point records of their
// chunk of 64 evaluation points, and where the two partial records wait for them in LDS.  Integers only; a plain host
// compiler builds the same text for the CPU tests (tests/cpp/rec_pieces_shim.cpp).
//
// A record holds RECL = NG + D + 1 values and starts every RECS doubles (RECS even, >= RECL).  It is stored as
// npieces = (RECL + 1) / 2 pairs of doubles; the last pair of an odd RECL carries a 0.0 pad.  Piece e of a chunk is point
// e / npieces, pair e % npieces: with RECS = 2 npieces (every arm plan) consecutive pieces are consecutive 16 bytes of
// memory, so that 64 lanes that take 64 consecutive pieces store one 1-KiB run.  Only the points below P.P exist: the
// live points of a chunk are its first `live`, and the pieces are 0 .. live * npieces - 1.
#pragma once

#ifndef G2_PURE
#ifdef __HIPCC__
#define G2_PURE __host__ __device__ __forceinline__
#else
#define G2_PURE inline
#endif
#endif

namespace g2 {

G2_PURE constexpr int rec_npieces(int RECL) { return (RECL + 1) / 2; }
// points of the chunk that starts at point p_lo which exist (p < P): their records are the ones stored
G2_PURE int rec_live_points(int P, int p_lo) { return P - p_lo < 0 ? 0 : P - p_lo > 64 ? 64 : P - p_lo; }
G2_PURE int rec_piece_count(int live, int RECL) { return live * rec_npieces(RECL); }

// A partial record in LDS is point-major as well: point pt keeps its RECL values from pt * rec_lds_stride(RECL) on.  The
// stride is odd, so that 64 lanes that each write value k of their own point, and 64 lanes that read consecutive pieces,
// spread over the banks (a stride of 64 doubles -- value-major -- would put the 18 pieces of a point on one bank).
G2_PURE constexpr int rec_lds_stride(int RECL) { return RECL | 1; }

struct RecPiece {
  int point, pair;       // point of the chunk 0 .. 63; the piece holds the values 2 pair and 2 pair + 1 of its record
  bool padded;           // value 2 pair + 1 does not exist (odd RECL, last pair): 0.0 is stored in its place
  long dst;              // first double of the piece, counted from the record of the chunk's first point
  int src;               // value 2 pair of the point in a partial record in LDS, counted from the partial's start
};
G2_PURE RecPiece rec_piece(int e, int RECL, int RECS) {
  const int np = rec_npieces(RECL), point = e / np, pair = e - point * np;
  return RecPiece{point, pair, 2 * pair + 1 >= RECL, (long)point * RECS + 2 * pair, point * rec_lds_stride(RECL) + 2 * pair};
}

}  // namespace g2
