// fx_shapes.h — shape constants of the fx / fxl kernels (kernels_fx.hip) that the host's layout
// arithmetic needs too, and that arithmetic.  Host-only: no HIP includes.
#pragma once

constexpr int FX_DROW = 256;  // delta0 digit image: 16 rows x 16 B per K group (read twice per tile)
constexpr int FXL_MAXW = 8;   // fxl: waves per workgroup at most

// dynamic LDS of an fxl workgroup of nw waves, nl layers, cpw chunks per wave
inline int fxl_lds_bytes(int nw, int nl, int cpw) {
  const int ns = 8 + (nl - 2) * 20;
  return nw * (2 * cpw * 1024 + 4 * FX_DROW + 2 * 64 * 16) + 2 * 64 * 4 + nl * 20 * 4 + ns * 4;
}

// marker chunks per fxl wave: 4 up to 32 chunks, else 8; force = 8 (EnvOptions::fxl_cpw): always 8,
// the old scheme (A/B)
inline int fxl_cpw(int nchunks, int force) { return (nchunks <= 4 * FXL_MAXW && force != 8) ? 4 : 8; }
