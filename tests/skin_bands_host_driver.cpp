// The skin-band rule of the pair rows (scema_amd/csrc/md_skin_bands.h) compiled for the host: tests/test_skin_bands_rule.py calls it through
// ctypes.  The header is the one k_pair, k_initial_integrate and the engine's layout include.
#include "../scema_amd/csrc/md_skin_bands.h"

extern "C" {
int sbh_bands() { return MD_SKIN_BANDS; }
int sbh_levels() { return MD_DLEVELS; }
float sbh_up(double v) { return skin_up(v); }
float sbh_down(double v) { return skin_down(v); }
int sbh_level(float d_up, float inv_quantum) { return skin_level(d_up, inv_quantum); }
float sbh_level_bound(int level, float quantum) { return skin_level_bound(level, quantum); }
int sbh_open(float d_i, float d_g, float corner, const float *w) { return skin_bands_open(d_i, d_g, corner, w); }
}
