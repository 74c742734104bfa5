// Axis-symmetric tool tasks through the C++ mirror (include/loik_amd/loik.hpp: setPoseTasks with LOIKB_TASK_POSE_AXIS / LOIKB_TASK_AXIS;
// include/loik_amd_axis.h): Panda-7, a tool frame on the last link, the target spun about its own z axis by one radian.
// Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

static_assert(LOIKB_TASK_FREE_Z == 4 && LOIKB_TASK_POSE_AXIS == 4 && LOIKB_TASK_AXIS == 6, "the kinds of loik_amd_axis.h");
static_assert(LOIKB_TASK_POSE_AXIS == (LOIKB_TASK_POSE | LOIKB_TASK_FREE_Z) && LOIKB_TASK_AXIS == (LOIKB_TASK_ORIENTATION | LOIKB_TASK_FREE_Z), "a modifier bit");

int main()
{
  int failures = 0;
  if (loikb_axis_version() != LOIKB_AXIS_VERSION) { ++failures; std::printf("loikb_axis_version() = %d, header %d\n", loikb_axis_version(), LOIKB_AXIS_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 64;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec q_t(model.nq, 0.3), q0((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) q0[(std::size_t)b * model.nq + k] = 0.3 + 0.1 * std::sin(1.0 + b + 7.0 * k);
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  // the tool frame: a quarter turn about z, 0.1 along x and 0.12 along z of the link
  const SE3 tool{0, -1, 0, 1, 0, 0, 0, 0, 1, 0.1, 0.0, 0.12};
  solver.SolveInit(q_t, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  // the target: the tool frame at q = 0.3 everywhere, spun about its own z by one radian (columns x and y turn, z and t stay)
  const SE3 F = solver.FramePlacements({ee}, {tool})[0];
  SE3 D = F;
  const double c = std::cos(1.0), s = std::sin(1.0);
  for (int r = 0; r < 3; ++r) {
    D[3 * r] = c * F[3 * r] + s * F[3 * r + 1];
    D[3 * r + 1] = -s * F[3 * r] + c * F[3 * r + 1];
  }
  for (int what = 0; what < 2; ++what) {
    const int kind = what == 0 ? LOIKB_TASK_POSE_AXIS : LOIKB_TASK_AXIS;
    solver.setPoseTasks({kind}, {tool});
    const auto tasks = solver.PoseTasks();
    if (tasks.size() != 1 || tasks[0].first != kind || tasks[0].second != tool) { ++failures; std::printf("PoseTasks does not return what was set\n"); }
    const FirstOrderLoikOptimized::PoseResult r = solver.SolvePose({D}, 1.0, 1.0, 1e-6, 20, &q0);
    const std::vector<SE3> Fq = solver.FramePlacements(std::vector<Index>(1, ee), {tool});
    int reached = 0, spin_free = 0, unmasked = 0;
    for (int b = 0; b < B; ++b) {
      reached += r.reached[b];
      unmasked += r.err[(std::size_t)b * 6 + 5] != 0.0;
      if (what == 1)
        for (int k = 0; k < 3; ++k) unmasked += r.err[(std::size_t)b * 6 + k] != 0.0;
      if (!r.reached[b]) continue;
      double dz = 0, dp = 0, dx = 0;
      for (int k = 0; k < 3; ++k) {
        dz = std::fmax(dz, std::fabs(Fq[b][3 * k + 2] - D[3 * k + 2]));   // the z axis: the third column
        dx = std::fmax(dx, std::fabs(Fq[b][3 * k] - D[3 * k]));           // the x axis: where the spin shows
        dp = std::fmax(dp, std::fabs(Fq[b][9 + k] - D[9 + k]));
      }
      // reached in the task's part (world-frame differences are the frame-axis ones up to a rotation: sqrt(3) covers it) ...
      if (dz > 2e-6) { ++failures; std::printf("instance %d reached but its z axis is %.3e off\n", b, dz); }
      if (what == 0 && dp > 2e-6) { ++failures; std::printf("instance %d reached but its origin is %.3e off\n", b, dp); }
      // ... and the spin was left free: nobody turned the tool by the radian
      spin_free += dx > 1e-4;
    }
    if (unmasked) { ++failures; std::printf("task %d: %d entries of err outside the mask are not zero\n", kind, unmasked); }
    if (reached < B * 9 / 10) { ++failures; std::printf("task %d: only %d of %d reached\n", kind, reached, B); }
    if (spin_free < reached / 2) { ++failures; std::printf("task %d: the spin matches the target on %d of %d\n", kind, reached - spin_free, reached); }
    std::printf("task %d: %d of %d reached, %d of them with the spin off the target's\n", kind, reached, B, spin_free);
  }
  // the kinds that mean nothing throw and leave the specification in place
  {
    int n_threw = 0;
    for (int bad : {3, 5, 7, 8, -1}) {
      try { solver.setPoseTasks({bad}, {tool}); } catch (const std::runtime_error&) { ++n_threw; }
    }
    if (n_threw != 5) { ++failures; std::printf("%d of 5 bad kinds threw\n", n_threw); }
    const auto tasks = solver.PoseTasks();
    if (tasks.size() != 1 || tasks[0].first != LOIKB_TASK_AXIS) { ++failures; std::printf("a rejected specification changed the handle\n"); }
  }
  if (failures) return 1;
  std::printf("all axis tasks checks passed\n");
  return 0;
}
