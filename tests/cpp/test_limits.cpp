// Joint position limits through the C++ mirror (include/loik_amd/loik.hpp: setJointLimits, UpdateIneqConstraints, PoseLimitFlags;
// include/loik_amd_limits.h): Panda-7, seeds around one configuration, a target the limits keep out of reach for the elbow.
// Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

using namespace loik_amd;

int main()
{
  const Model model = Model::Builtin("panda7");
  const int B = 64;
  const Index ee = 7;
  const double inf = std::numeric_limits<double>::infinity();
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec q_t(model.nq, 0.3), q0((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) q0[(std::size_t)b * model.nq + k] = 0.1 + 0.05 * std::sin(1.0 + b + 7.0 * k);
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  int failures = 0;
  bool threw = false;
  try { solver.UpdateIneqConstraints(lb, ub); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("UpdateIneqConstraints before SolveInit did not throw\n"); }
  solver.SolveInit(q_t, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const FirstOrderLoikOptimized::SE3 target = solver.ForwardKinematics({ee})[0];   // the placement at q = 0.3 everywhere
  // every joint must stay below 0.2: the target (reached at 0.3) is out of range for most of them
  DVec q_lo(model.nv, -inf), q_hi(model.nv, 0.2);
  solver.setJointLimits(q_lo, q_hi);
  const FirstOrderLoikOptimized::PoseResult r = solver.SolvePose({target}, 0.5, 0.5, 1e-6, 12, &q0);
  const DVec q = solver.q_resident();
  const std::vector<int> flags = solver.PoseLimitFlags();
  int flagged = 0, resting = 0, reached = 0;
  for (int b = 0; b < B; ++b) {
    reached += r.reached[b];
    for (int k = 0; k < model.nv; ++k) {
      const double x = q[(std::size_t)b * model.nq + k];
      if (!(x <= 0.2)) { ++failures; std::printf("instance %d joint %d at %.17g above its limit\n", b, k, x); }
      resting += x == 0.2;
      flagged += (flags[(std::size_t)b * model.nv + k] & LOIKB_LIMIT_UPPER) != 0;
      if (flags[(std::size_t)b * model.nv + k] & LOIKB_LIMIT_LOWER) { ++failures; std::printf("a lower flag without a lower limit\n"); }
    }
  }
  if (!resting || !flagged) { ++failures; std::printf("the limits never bound (%d resting, %d flagged)\n", resting, flagged); }
  // a finite limit where none can be: the (x, y, z, quaternion) of a free-flyer has no scalar coordinate per DoF -- Panda has none,
  // so the wrong size is what this model can show; NaN and an empty range as well
  for (int what = 0; what < 3; ++what) {
    DVec lo2(model.nv + (what == 0), -inf), hi2(model.nv + (what == 0), inf);
    if (what == 1) lo2[2] = std::nan("");
    if (what == 2) { lo2[2] = 1.0; hi2[2] = 0.0; }
    threw = false;
    try { solver.setJointLimits(lo2, hi2); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { ++failures; std::printf("bad limits (%d) did not throw\n", what); }
  }
  // cleared: the same seeds reach the target, and the flags are gone
  solver.clearJointLimits();
  const FirstOrderLoikOptimized::PoseResult r2 = solver.SolvePose({target}, 0.5, 0.5, 1e-6, 40, &q0);
  int reached2 = 0;
  for (int b = 0; b < B; ++b) reached2 += r2.reached[b];
  if (reached2 < B / 2) { ++failures; std::printf("without limits only %d of %d reached\n", reached2, B); }
  threw = false;
  try { (void)solver.PoseLimitFlags(); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("PoseLimitFlags after a solve without limits did not throw\n"); }
  // a tighter velocity box through UpdateIneqConstraints holds in the next Solve()
  DVec lb2(model.nv, -0.01), ub2(model.nv, 0.01);
  solver.UpdateIneqConstraints(lb2, ub2);
  solver.UpdateEqConstraint(ee, std::vector<Vec6>{Vec6{1.0, 1.0, 1.0, 1.0, 1.0, 1.0}});
  solver.Solve();
  DVec z((std::size_t)B * model.nv);
  if (loikb_get(solver.handle(), LOIKB_F_Z, z.data(), 0) != 0) { ++failures; std::printf("loikb_get(z) failed\n"); }
  int at_bound = 0;
  for (double v : z) {
    if (std::fabs(v) > 0.01) { ++failures; std::printf("z = %.17g outside the updated box\n", v); break; }
    at_bound += std::fabs(v) == 0.01;
  }
  if (!at_bound) { ++failures; std::printf("the updated box never binds\n"); }
  std::printf("%d reached with limits (%d coordinates resting on a limit, %d flagged), %d without\n", reached, resting, flagged, reached2);
  if (failures) return 1;
  std::printf("all limits checks passed\n");
  return 0;
}
