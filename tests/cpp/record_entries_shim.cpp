// C entry points around gpmp2_amd/csrc/record_entries.h for the CPU tests (tests/test_record_entries_cpu.py): the map
// from a packed record entry to its two row positions, built by the host compiler alone.  Nothing else lives here.
#include "record_entries.h"

#include "../../include/gpmp2mi.h"

extern "C" {

int shim_record_entries(int D, int NG) { return g2::record_entries(D, NG); }

void shim_record_entry(int D, int NG, int e, int* ea, int* eb) { g2::record_entry(D, NG, e, *ea, *eb); }

int shim_rec_slots() { return g2::REC_SLOTS; }

int shim_max_dof() { return GPMP2MI_MAX_DOF; }

}  // extern "C"
