// md_row_entry.h -- the format of one entry of a full neighbour row (built by k_row_build, md_rows.hip), for device and host code alike:
// plain macros, so that the arithmetic headers g++ compiles for the CPU tests (sw/sw_core.h) can name it.
#pragma once

#define ROW_CODE0 62         /* row entry: [23:0] atom, [30:24] image code (sx+2) + 5 (sy+2) + 25 (sz+2), as the ReaxFF rows (RX_JMASK); 62 = no shift */
#define ROW_JMASK 0x00FFFFFF
#define ROW_NSHIFT 125       /* image codes: 5 x 5 x 5 */
