// Voxel worlds through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_grid.h): Panda-7, two spheres per link, a
// world of two spheres, one box and a grid of 9 x 8 x 7 voxels of 1/8, self pairs; the configurations and displacements of
// tests/cpp/test_motion.cpp.  With a path as its argument the program writes the distance field and what Clearance and MotionClearance
// returned there (raw doubles, the integers as doubles), for tests/test_cpp_grid.py to compare with the Python binding bit for bit.
// Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_GRID_VERSION == 1, "the version of loik_amd_grid.h");
static_assert(LOIKB_CLR_WORLD_GRID == LOIKB_CLR_SELF + 1, "the witness kind follows those of loik_amd_collision.h");

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_grid_version() != LOIKB_GRID_VERSION) { ++failures; std::printf("loikb_grid_version() = %d, header %d\n", loikb_grid_version(), LOIKB_GRID_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  // configurations and displacements that are the same doubles in any language: sixteenths and sixty-fourths
  DVec qa((std::size_t)B * model.nq), dv((std::size_t)B * model.nv);
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
    for (int k = 0; k < model.nv; ++k) dv[(std::size_t)b * model.nv + k] = ((b * 5 + 11 * k) % 23 - 11) / 64.0;
  }
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
  if (solver.GetCollisionGrid()) { ++failures; std::printf("a grid before one was set\n"); }
  const auto before = solver.Clearance();
  const std::array<int, 3> dims{{9, 8, 7}};
  const std::array<double, 3> origin{{-0.5, -0.5, 0.0}};
  const double voxel = 0.125;
  std::vector<unsigned char> occ((std::size_t)dims[0] * dims[1] * dims[2]);
  int filled = 0;
  for (int z = 0; z < dims[2]; ++z)
    for (int y = 0; y < dims[1]; ++y)
      for (int x = 0; x < dims[0]; ++x) filled += (occ[((std::size_t)z * dims[1] + y) * dims[0] + x] = (unsigned char)((x * 7 + y * 5 + z * 3) % 23 == 0));
  solver.SetCollisionGrid(occ, dims, origin, voxel);
  FirstOrderLoikOptimized::CollisionGrid g;
  if (!solver.GetCollisionGrid(&g) || g.dims != dims || g.origin != origin || g.voxel != voxel || g.G.size() != occ.size()) { ++failures; std::printf("GetCollisionGrid\n"); }
  // the field against the brute force
  for (int z = 0; z < dims[2] && !failures; ++z)
    for (int y = 0; y < dims[1]; ++y)
      for (int x = 0; x < dims[0]; ++x) {
        unsigned int best = LOIKB_GRID_EMPTY;
        for (int uz = 0; uz < dims[2]; ++uz)
          for (int uy = 0; uy < dims[1]; ++uy)
            for (int ux = 0; ux < dims[0]; ++ux) {
              if (!occ[((std::size_t)uz * dims[1] + uy) * dims[0] + ux]) continue;
              unsigned int v = 0;
              for (int d : {x - ux, y - uy, z - uz}) { const unsigned int a = (unsigned int)std::abs(d); v += a ? (2 * a - 1) * (2 * a - 1) : 0u; }
              if (v < best) best = v;
            }
        if (g.G[((std::size_t)z * dims[1] + y) * dims[0] + x] != best) { ++failures; std::printf("G at (%d, %d, %d)\n", x, y, z); }
      }
  const auto clr = solver.Clearance();
  const double margin = -0.0625, tol = 1.0 / 1024;
  const auto mot = solver.MotionClearance(qa, dv, margin, tol, 16);
  int grid_wit = 0, lower = 0;
  for (int b = 0; b < B; ++b) {
    if (clr.min[b] != std::fmin(clr.min_world[b], clr.min_self[b])) { ++failures; std::printf("configuration %d: min\n", b); }
    if (clr.min_world[b] > before.min_world[b] || clr.min_self[b] != before.min_self[b]) { ++failures; std::printf("configuration %d: the grid raised a minimum\n", b); }
    lower += clr.min_world[b] < before.min_world[b];
    if (clr.witness[3 * (std::size_t)b] == LOIKB_CLR_WORLD_GRID) {
      ++grid_wit;
      const int a = clr.witness[3 * (std::size_t)b + 1], v = clr.witness[3 * (std::size_t)b + 2];
      if (a < 0 || a >= (int)links.size() || v < 0 || v >= (int)occ.size()) { ++failures; std::printf("configuration %d: the witness\n", b); }
    }
  }
  if (filled == 0 || grid_wit == 0 || lower == 0) { ++failures; std::printf("the grid decides nothing: %d voxels, %d witnesses, %d minima\n", filled, grid_wit, lower); }
  // avoidance refuses a voxel world, a bad grid is refused, and a cleared grid is no grid
  int n_threw = 0;
  try { solver.SetCollisionAvoidance(0.01, 0.1); } catch (const std::runtime_error&) { ++n_threw; }
  try { solver.SetCollisionGrid(occ, dims, origin, 0.0); } catch (const std::runtime_error&) { ++n_threw; }
  try { solver.SetCollisionGrid(occ, {{9, 8, 6}}, origin, voxel); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 3) { ++failures; std::printf("%d of 3 bad calls threw\n", n_threw); }
  solver.ClearCollisionGrid();
  const auto after = solver.Clearance();
  if (solver.GetCollisionGrid() || after.min != before.min || after.witness != before.witness) { ++failures; std::printf("a cleared grid left something\n"); }
  DVec all(g.G.begin(), g.G.end());
  for (const DVec* v : {&clr.min, &clr.min_world, &clr.min_self}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), clr.witness.begin(), clr.witness.end());
  all.insert(all.end(), mot.status.begin(), mot.status.end());
  all.insert(all.end(), mot.evals.begin(), mot.evals.end());
  for (const DVec* v : {&mot.s_free, &mot.min_sampled, &mot.s_at_min}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), mot.witness.begin(), mot.witness.end());
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all grid checks passed\n");
  return 0;
}
