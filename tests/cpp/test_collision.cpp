// Collision clearance through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_collision.h): Panda-7, two
// spheres per link, a world of two spheres and one box, self pairs.  With a path as its argument the program writes what Clearance
// returned there (raw doubles: min, min_world, min_self, then the witnesses as doubles, of the resident q and of five explicit rows), for
// tests/test_cpp_collision.py to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_CLR_NONE == 0 && LOIKB_CLR_WORLD_SPHERE == 1 && LOIKB_CLR_WORLD_BOX == 2 && LOIKB_CLR_SELF == 3, "the witness kinds of loik_amd_collision.h");
static_assert(LOIKB_MS_GOAL_IN_COLLISION == 8 && LOIKB_CLR_MS_F_INSTANCE == 3, "the goal status and the result fields");

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_collision_version() != LOIKB_COLLISION_VERSION) { ++failures; std::printf("loikb_collision_version() = %d, header %d\n", loikb_collision_version(), LOIKB_COLLISION_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  // configurations that are the same doubles in any language: sixteenths
  DVec q0((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) q0[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  bool threw = false;
  try { (void)solver.Clearance(); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("Clearance without spheres did not throw\n"); }
  solver.SolveInit(q0, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  // two spheres per link, offsets and radii in sixty-fourths
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
  // 14 spheres, 91 pairs: less 7 on the same link, 6 * 4 between parent and child, 4 ignored
  if (solver.NumSelfPairs() != 91 - 7 - 24 - 4) { ++failures; std::printf("NumSelfPairs() = %d\n", solver.NumSelfPairs()); }
  const auto r = solver.Clearance();
  const DVec five(q0.begin() + 3 * model.nq, q0.begin() + 8 * model.nq);
  const auto e = solver.Clearance(&five);
  if (r.min.size() != (std::size_t)B || r.witness.size() != 3 * (std::size_t)B || e.min.size() != 5) { ++failures; std::printf("Clearance returned %zu and %zu rows\n", r.min.size(), e.min.size()); }
  for (int b = 0; b < B; ++b) {
    if (!(r.min[b] == std::fmin(r.min_world[b], r.min_self[b]))) { ++failures; std::printf("instance %d: min is not min(min_world, min_self)\n", b); }
    if (r.witness[3 * b] < LOIKB_CLR_WORLD_SPHERE || r.witness[3 * b] > LOIKB_CLR_SELF || r.witness[3 * b + 1] < 0 || r.witness[3 * b + 1] >= 14) { ++failures; std::printf("instance %d: witness\n", b); }
  }
  for (int i = 0; i < 5; ++i)
    if (e.min[i] != r.min[3 + i] || e.witness[3 * i + 2] != r.witness[3 * (3 + i) + 2]) { ++failures; std::printf("row %d of an explicit q differs from the resident one\n", i); }
  DVec all;
  for (const auto* x : {&r, &e}) {
    all.insert(all.end(), x->min.begin(), x->min.end());
    all.insert(all.end(), x->min_world.begin(), x->min_world.end());
    all.insert(all.end(), x->min_self.begin(), x->min_self.end());
    all.insert(all.end(), x->witness.begin(), x->witness.end());
  }
  // the latch
  double margin = -1.0;
  if (solver.MultiStartClearance()) { ++failures; std::printf("a latch before any was set\n"); }
  solver.setMultiStartClearance(0.03125);
  if (!solver.MultiStartClearance(&margin) || margin != 0.03125) { ++failures; std::printf("the latch does not return what was set\n"); }
  int n_threw = 0;
  for (double bad : {std::nan(""), (double)INFINITY}) {
    try { solver.setMultiStartClearance(bad); } catch (const std::runtime_error&) { ++n_threw; }
  }
  if (n_threw != 2 || !solver.MultiStartClearance(&margin) || margin != 0.03125) { ++failures; std::printf("%d of 2 bad margins threw, latch %g\n", n_threw, margin); }
  solver.clearMultiStartClearance();
  if (solver.MultiStartClearance()) { ++failures; std::printf("the latch was not cleared\n"); }
  // a bad model is refused and the one in force answers as before
  threw = false;
  try { solver.setCollisionSpheres({ee}, {0.0, 0.0, 0.0, -1.0}); } catch (const std::runtime_error&) { threw = true; }
  if (!threw || solver.Clearance().min != r.min) { ++failures; std::printf("a negative radius was accepted, or changed the model\n"); }
  // an empty world and no pairs: +inf, no witness
  solver.setCollisionWorld();
  solver.setSelfCollision(false);
  const auto none = solver.Clearance();
  if (!(std::isinf(none.min[0]) && none.min[0] > 0 && none.witness[0] == LOIKB_CLR_NONE && none.witness[1] == -1 && none.witness[2] == -1)) { ++failures; std::printf("an empty set of pairs\n"); }
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all collision checks passed\n");
  return 0;
}
