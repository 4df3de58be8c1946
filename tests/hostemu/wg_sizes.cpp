// Host definitions of the workgroup program's LDS sizing (vertex_wg.hip defines the same two entry points for the device library), for
// tests/hostemu/plan_emu.cpp.  Built twice like vertex_wg.hip: as is (256 threads) and with build.py's T512 flags (512 threads, _t512 names).
#include "vertex_wg.h"

#ifndef GCS_WG_SYM
#define GCS_WG_SYM(name) name
#endif

int GCS_WG_SYM(gcsadmm_wg_lds_bytes)(int n, int units, int facets, bool box) { return 8 * gcs_wg::wg_lds_doubles_n(n, units, facets, box); }
bool GCS_WG_SYM(gcsadmm_wg_has_box)(int n) { return gcs_wg::wg_has_box(n); }
