// tests/eq_host_shim.cpp — TEST HARNESS ONLY. The host build of ground-fusion2_amd/csrc/gfbe_eq.h behind a C interface, so that
// tests/test_eq_model.py can hold the same text the device compiles against the model tests/eq_np.py, bit for bit.
#include "../ground-fusion2_amd/csrc/gfbe_eq.h"

using namespace gfd;

extern "C" {

// 1: the geometry is refused
int shim_eq_refused(int rows, int cols, int tiles_x, int tiles_y, double clip_limit) { return eq_geom_error(rows, cols, tiles_x, tiles_y, clip_limit) != nullptr; }

// ints [3] = tw, th, limit; floats [3] = scale, inv_tw, inv_th
void shim_eq_geom(int rows, int cols, int tiles_x, int tiles_y, double clip_limit, int *ints, float *floats) {
  const EqGeom g = eq_geom(rows, cols, tiles_x, tiles_y, clip_limit);
  ints[0] = g.tw; ints[1] = g.th; ints[2] = g.limit;
  floats[0] = g.scale; floats[1] = g.inv_tw; floats[2] = g.inv_th;
}

// lut [tiles_y][tiles_x][256]; out [rows][cols], which may be img
void shim_eq(const uint8_t *img, int rows, int cols, int tiles_x, int tiles_y, double clip_limit, uint8_t *lut, uint8_t *out) {
  const EqGeom g = eq_geom(rows, cols, tiles_x, tiles_y, clip_limit);
  eq_host_lut(img, g, lut);
  eq_host_apply(img, g, lut, out);
}

// bin i of a histogram after E3, given the sum of the excesses
int shim_eq_redistribute(int bin, int i, int limit, int clipped) { return eq_redistribute(bin, i, limit, clipped); }

}  // extern "C"
