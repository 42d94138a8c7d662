// fx_shapes.h — shape constants of the fx / fxl / fxh kernels (kernels_fx.hip, kernels_fxl.hip,
// kernels_fxh.hip) that the host's layout arithmetic needs too, and that arithmetic.  Host-only: no
// HIP includes.
#pragma once

constexpr int FX_DROW = 256;  // delta0 digit image: 16 rows x 16 B per K group (read twice per tile)
constexpr int FXL_MAXW = 8;   // fxl: waves per workgroup at most
constexpr int FXH_CPW = 5;    // fxh: chunks per compute wave (at most)
constexpr int FXH_MAXC = 7;   // fxh: compute waves (+ the head wave: 8 waves)
constexpr int FXH_NSL = 4;    // fxh: genotype slots per compute wave

// dynamic LDS of an fxl workgroup of nw waves, nl layers, cpw chunks per wave
inline int fxl_lds_bytes(int nw, int nl, int cpw) {
  const int ns = 8 + (nl - 2) * 20;
  return nw * (2 * cpw * 1024 + 4 * FX_DROW + 2 * 64 * 16) + 2 * 64 * 4 + nl * 20 * 4 + ns * 4;
}

// marker chunks per fxl wave: 4 up to 32 chunks, else 8; force = 8 (EnvOptions::fxl_cpw): always 8,
// the old scheme (A/B)
inline int fxl_cpw(int nchunks, int force) { return (nchunks <= 4 * FXL_MAXW && force != 8) ? 4 : 8; }

// dynamic LDS of an fxh workgroup of nc compute waves, nl layers; slot_kib: the largest chunk count of
// a compute wave (one KiB per chunk and slot)
inline int fxh_lds_bytes(int nc, int nl, int slot_kib) {
  const int ns = 8 + (nl - 2) * 20;
  return nc * FXH_NSL * slot_kib * 1024 + 2 * nc * 64 * 16 + 2 * 4 * FX_DROW + 3 * 64 * 4 + 16 * 4 + nl * 20 * 4 +
         ns * 4 + 4 * 4;
}

// the head-wave kernel takes the fxl groups of 4-chunk waves with >= 5 waves (17 .. 32 chunks);
// head = the context's choice (EnvOptions::fxl_head, read once at context creation:
// BANN_FXL_HEAD=0 keeps fxl for A/B), part of the launch group and its graph key
inline bool fxh_takes(int nw, int cpw, int head) { return head && cpw == 4 && nw >= 5 && nw <= 8; }
