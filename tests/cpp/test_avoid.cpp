// Collision avoidance through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_avoid.h): Panda-7, two spheres per
// link, a world of two spheres and one box, self pairs.  With a path as its argument the program writes what ClearanceGradient,
// AvoidanceBox and a SolvePose with the latch returned there (raw doubles, the integers as doubles), for tests/test_cpp_avoid.py to
// compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_AVOID_F_MIN_SEEN == 0 && LOIKB_AVOID_F_ACTIVE_STEPS == 1 && LOIKB_AVOID_F_FLAGS == 2, "the fields of loik_amd_avoid.h");
static_assert(sizeof(loikb_avoid_params) == 32, "three doubles and an int");
static_assert(LOIKB_AVOID_MAX_SPHERES >= 256, "the limit of loik_amd_avoid.h");

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_avoid_version() != LOIKB_AVOID_VERSION) { ++failures; std::printf("loikb_avoid_version() = %d, header %d\n", loikb_avoid_version(), LOIKB_AVOID_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec qa((std::size_t)B * model.nq);   // the same doubles in any language: sixteenths
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  const double d_safe = 1.0 / 64, d_influence = 0.25, kappa = 0.5, dt = 0.25;
  int n_threw = 0;
  try { solver.SetCollisionAvoidance(d_safe, d_influence, kappa); } catch (const std::runtime_error&) { ++n_threw; }   // no spheres yet
  solver.SolveInit(qa, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  try { (void)solver.ClearanceGradient(); } catch (const std::runtime_error&) { ++n_threw; }
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
  try { solver.SetCollisionAvoidance(d_safe, d_safe, kappa); } catch (const std::runtime_error&) { ++n_threw; }          // d_influence <= d_safe
  try { solver.SetCollisionAvoidance(d_safe, d_influence, 0.0); } catch (const std::runtime_error&) { ++n_threw; }       // kappa
  try { (void)solver.AvoidanceBox(nullptr, 0.0, lb, ub, d_safe, d_influence, kappa); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.AvoidanceResult(); } catch (const std::runtime_error&) { ++n_threw; }                               // no pose loop yet
  if (n_threw != 6) { ++failures; std::printf("%d of 6 bad calls threw\n", n_threw); }
  if (solver.CollisionAvoidance()) { ++failures; std::printf("a refused latch is set\n"); }

  const auto g = solver.ClearanceGradient();
  const auto c = solver.Clearance();
  const std::size_t nv = (std::size_t)model.nv, ns = links.size();
  if (g.grad.size() != B * nv || g.clearance.min != c.min || g.clearance.witness != c.witness) { ++failures; std::printf("ClearanceGradient against Clearance\n"); }
  const auto box = solver.AvoidanceBox(&qa, dt, lb, ub, d_safe, d_influence, kappa);
  if (box.lo.size() != B * nv || box.pairs.size() != 2 * B * ns || box.partner.size() != 2 * B * ns) { ++failures; std::printf("AvoidanceBox sizes\n"); }
  int narrowed = 0;
  for (std::size_t i = 0; i < box.lo.size(); ++i) {
    if (!(box.lo[i] >= lb[i % nv] && box.lo[i] <= 0.0 && box.hi[i] >= 0.0 && box.hi[i] <= ub[i % nv])) { ++failures; std::printf("AvoidanceBox: entry %zu\n", i); break; }
    narrowed += box.lo[i] > lb[i % nv] || box.hi[i] < ub[i % nv];
  }
  if (!narrowed) { ++failures; std::printf("AvoidanceBox narrowed nothing\n"); }

  // a pose loop with the latch: the box of its first step is the one above
  solver.SetCollisionAvoidance(d_safe, d_influence, kappa);
  loikb_avoid_params got{};
  if (!solver.CollisionAvoidance(&got) || got.d_safe != d_safe || got.d_influence != d_influence || got.kappa != kappa) { ++failures; std::printf("CollisionAvoidance()\n"); }
  const FirstOrderLoikOptimized::SE3 target{1, 0, 0, 0, 1, 0, 0, 0, 1, 0.375, 0.125, 0.5};
  const auto pose = solver.SolvePose({target}, dt, 0.5, 1e-4, 2, &qa);
  const auto res = solver.AvoidanceResult();
  int active = 0;
  for (int b = 0; b < B; ++b) {
    active += res.active_steps[b] > 0;
    if (pose.steps[b] > 0 && !(res.min_seen[b] <= g.clearance.min[b])) { ++failures; std::printf("instance %d: min_seen %g above the clearance of its seed %g\n", b, res.min_seen[b], g.clearance.min[b]); }
    if (res.active_steps[b] < 0 || res.active_steps[b] > pose.steps[b]) { ++failures; std::printf("instance %d: active_steps\n", b); }
  }
  if (!active) { ++failures; std::printf("the latch narrowed no step\n"); }
  solver.ClearCollisionAvoidance();
  if (solver.CollisionAvoidance()) { ++failures; std::printf("ClearCollisionAvoidance()\n"); }

  DVec all(g.grad);
  all.insert(all.end(), g.clearance.min.begin(), g.clearance.min.end());
  all.insert(all.end(), g.clearance.witness.begin(), g.clearance.witness.end());
  all.insert(all.end(), box.lo.begin(), box.lo.end());
  all.insert(all.end(), box.hi.begin(), box.hi.end());
  all.insert(all.end(), box.pairs.begin(), box.pairs.end());
  all.insert(all.end(), box.partner.begin(), box.partner.end());
  all.insert(all.end(), res.min_seen.begin(), res.min_seen.end());
  all.insert(all.end(), res.active_steps.begin(), res.active_steps.end());
  all.insert(all.end(), res.flags.begin(), res.flags.end());
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all avoidance checks passed\n");
  return 0;
}
