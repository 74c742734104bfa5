// The nearest-voxel transform through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_gridnear.h): the robot,
// spheres, world and grid of tests/cpp/test_grid.cpp.  With a path as its argument the program writes the transform and what GridNearest,
// ClearanceGradient and AvoidanceBox returned there (raw doubles, the integers as doubles), for tests/test_cpp_gridnear.py to compare with
// the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_GRIDNEAR_VERSION == 1, "the version of loik_amd_gridnear.h");
static_assert(LOIKB_GRID_NO_VOXEL == 0xFFFFFFFFu, "no voxel");

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_gridnear_version() != LOIKB_GRIDNEAR_VERSION) { ++failures; std::printf("loikb_gridnear_version() = %d\n", loikb_gridnear_version()); }
  const Model model = Model::Builtin("panda7");
  const int B = 67;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec qa((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(qa, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  std::vector<Index> links;
  DVec spheres;
  for (int l = 1; l <= 7; ++l)
    for (int k = 0; k < 2; ++k) {
      links.push_back(l);
      for (double v : {((l + k) % 5 - 2) / 64.0, ((2 * l + k) % 7 - 3) / 64.0, (k ? 4 : -3) / 64.0, (2 + (l + k) % 3) / 64.0}) spheres.push_back(v);
    }
  solver.setCollisionSpheres(links, spheres);
  solver.setCollisionWorld({0.25, 0.0, 0.5, 0.125, -0.5, 0.25, 0.25, 0.0625}, {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.0, 0.0, -0.25, 1.0, 1.0, 0.125});
  solver.setSelfCollision(true, {{2, 4}});
  const std::array<int, 3> dims{{9, 8, 7}};
  const std::array<double, 3> origin{{-0.5, -0.5, 0.0}};
  const double voxel = 0.125;
  std::vector<unsigned char> occ((std::size_t)dims[0] * dims[1] * dims[2]);
  for (int z = 0; z < dims[2]; ++z)
    for (int y = 0; y < dims[1]; ++y)
      for (int x = 0; x < dims[0]; ++x) occ[((std::size_t)z * dims[1] + y) * dims[0] + x] = (unsigned char)((x * 7 + y * 5 + z * 3) % 23 == 0);
  solver.SetCollisionGrid(occ, dims, origin, voxel);
  // without the latch: no transform, no query, and avoidance refuses the grid
  int n_threw = 0;
  if (solver.GetCollisionGridNearest()) { ++failures; std::printf("a transform before the latch\n"); }
  try { solver.GridNearest({0.0, 0.0, 0.25, 0.0625}); } catch (const std::runtime_error&) { ++n_threw; }
  try { solver.ClearanceGradient(); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 2) { ++failures; std::printf("%d of 2 calls without the latch threw\n", n_threw); }
  solver.SetCollisionGridNearest();
  std::vector<unsigned int> F;
  if (!solver.GetCollisionGridNearest(&F) || F.size() != occ.size()) { ++failures; std::printf("GetCollisionGridNearest\n"); }
  // the transform against the brute force: ascending index, replaced only by a strictly nearer voxel
  for (int z = 0; z < dims[2] && !failures; ++z)
    for (int y = 0; y < dims[1]; ++y)
      for (int x = 0; x < dims[0]; ++x) {
        unsigned int best = LOIKB_GRID_EMPTY, at = LOIKB_GRID_NO_VOXEL;
        for (int uz = 0; uz < dims[2]; ++uz)
          for (int uy = 0; uy < dims[1]; ++uy)
            for (int ux = 0; ux < dims[0]; ++ux) {
              const unsigned int u = (unsigned int)((uz * dims[1] + uy) * dims[0] + ux);
              if (!occ[u]) continue;
              unsigned int v = 0;
              for (int d : {x - ux, y - uy, z - uz}) { const unsigned int a = (unsigned int)std::abs(d); v += a ? (2 * a - 1) * (2 * a - 1) : 0u; }
              if (v < best) { best = v; at = u; }
            }
        if (F[((std::size_t)z * dims[1] + y) * dims[0] + x] != at) { ++failures; std::printf("F at (%d, %d, %d)\n", x, y, z); }
      }
  // the query: v <= d_u - r, a unit normal outside the cube, an occupied cube
  DVec qs;
  for (int i = 0; i < 40; ++i)
    for (double v : {((i * 7) % 19 - 9) / 16.0 + 1.0 / 256, ((i * 5) % 17 - 8) / 16.0 + 1.0 / 512, ((i * 3) % 13) / 16.0 + 3.0 / 1024, (i % 4) / 64.0}) qs.push_back(v);
  const auto nr = solver.GridNearest(qs);
  for (int i = 0; i < 40; ++i) {
    const double v = nr.val[2 * (std::size_t)i], up = nr.val[2 * (std::size_t)i + 1];
    const int u = nr.vox[2 * (std::size_t)i + 1];
    const double* n = &nr.normal[3 * (std::size_t)i];
    if (!(v <= up) || u < 0 || u >= (int)occ.size() || !occ[(std::size_t)u]) { ++failures; std::printf("sphere %d: the pair\n", i); }
    if (up + qs[4 * (std::size_t)i + 3] > 0.0 && std::fabs(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] - 1.0) > 1e-12) { ++failures; std::printf("sphere %d: the normal\n", i); }
  }
  // avoidance reads the grid
  const auto grad = solver.ClearanceGradient();
  const auto clr = solver.Clearance();
  if (grad.clearance.min != clr.min || grad.clearance.witness != clr.witness) { ++failures; std::printf("ClearanceGradient and Clearance differ\n"); }
  const auto box = solver.AvoidanceBox(nullptr, 0.25, lb, ub, 0.015625, 0.125, 0.5);
  const int nwo = 2 + 1;
  int grid_partner = 0;
  for (std::size_t k = 0; k < box.partner.size(); k += 2) grid_partner += box.partner[k] == nwo;
  if (grid_partner == 0) { ++failures; std::printf("no sphere has the grid as its nearest world object\n"); }
  solver.SetCollisionAvoidance(0.015625, 0.125);
  n_threw = 0;
  try { solver.SetCollisionGridNearest(false); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 1 || !solver.GetCollisionGridNearest()) { ++failures; std::printf("the latch went while avoidance reads the grid\n"); }
  solver.ClearCollisionAvoidance();
  solver.SetCollisionGridNearest(false);
  if (solver.GetCollisionGridNearest()) { ++failures; std::printf("a cleared latch left the transform\n"); }
  DVec all(F.begin(), F.end());
  all.insert(all.end(), nr.val.begin(), nr.val.end());
  all.insert(all.end(), nr.vox.begin(), nr.vox.end());
  all.insert(all.end(), nr.normal.begin(), nr.normal.end());
  all.insert(all.end(), grad.grad.begin(), grad.grad.end());
  for (const DVec* v : {&box.lo, &box.hi, &box.pairs}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), box.partner.begin(), box.partner.end());
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all gridnear checks passed\n");
  return 0;
}
