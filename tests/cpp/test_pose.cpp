// The pose layer of the C++ mirror (include/loik_amd/loik.hpp: SolvePose, ForwardKinematics, include/loik_amd_pose.h): Panda-7,
// a batch of seeds around one configuration whose end-effector placement is the target.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;

int main()
{
  const Model model = Model::Builtin("panda7");
  const int B = 64;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec q_t(model.nq, 0.3), q0((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) q0[(std::size_t)b * model.nq + k] = q_t[k] + 0.05 * std::sin(1.0 + b + 7.0 * k);
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(q_t, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const FirstOrderLoikOptimized::SE3 target = solver.ForwardKinematics({ee})[0];
  const FirstOrderLoikOptimized::PoseResult r = solver.SolvePose({target}, 1.0, 1.0, 1e-6, 20, &q0);
  int reached = 0, failures = 0;
  const std::vector<FirstOrderLoikOptimized::SE3> M = solver.ForwardKinematics({ee});
  for (int b = 0; b < B; ++b) {
    reached += r.reached[b];
    if (!r.reached[b]) continue;
    double d = 0.0;
    for (int k = 0; k < 12; ++k) d = std::fmax(d, std::fabs(M[b][k] - target[k]));
    if (d > 1e-5) { ++failures; std::printf("instance %d reached but %.3e from the target\n", b, d); }
  }
  if (reached < B / 2) { ++failures; std::printf("only %d of %d reached\n", reached, B); }
  bool threw = false;
  try { solver.SolvePose({target}, 0.0); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("dt = 0 did not throw\n"); }
  std::printf("%d of %d reached\n", reached, B);
  if (failures) return 1;
  std::printf("all pose checks passed\n");
  return 0;
}
