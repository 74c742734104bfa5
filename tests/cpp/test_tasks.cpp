// Tool frames and task kinds through the C++ mirror (include/loik_amd/loik.hpp: setPoseTasks, clearPoseTasks, PoseTasks,
// FramePlacements; include/loik_amd_tasks.h): Panda-7, a tool frame on the last link, a position task and an orientation task.
// Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

int main()
{
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
  int failures = 0;
  bool threw = false;
  try { solver.setPoseTasks({LOIKB_TASK_POSITION}, {tool}); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("setPoseTasks before SolveInit did not throw\n"); }
  solver.SolveInit(q_t, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  if (!solver.PoseTasks().empty()) { ++failures; std::printf("tasks on a fresh handle\n"); }
  // FramePlacements: oMf = oMi * iMf, checked entry by entry against ForwardKinematics (the batch holds q_t: one placement)
  const SE3 M = solver.ForwardKinematics({ee})[0], F = solver.FramePlacements({ee}, {tool})[0], F0 = solver.FramePlacements({ee})[0];
  for (int r = 0; r < 3; ++r) {
    double t = M[9 + r];
    for (int k = 0; k < 3; ++k) t += M[3 * r + k] * tool[9 + k];
    if (std::fabs(F[9 + r] - t) > 1e-12) { ++failures; std::printf("frame translation %d: %.17g, expected %.17g\n", r, F[9 + r], t); }
    for (int c = 0; c < 3; ++c) {
      double x = 0;
      for (int k = 0; k < 3; ++k) x += M[3 * r + k] * tool[3 * k + c];
      if (std::fabs(F[3 * r + c] - x) > 1e-12) { ++failures; std::printf("frame rotation %d %d\n", r, c); }
    }
  }
  if (F0 != M) { ++failures; std::printf("FramePlacements without frames is not ForwardKinematics\n"); }
  // the target: the tool frame at q = 0.3 everywhere
  for (int what = 0; what < 2; ++what) {
    const int kind = what == 0 ? LOIKB_TASK_POSITION : LOIKB_TASK_ORIENTATION;
    solver.setPoseTasks({kind}, {tool});
    const auto tasks = solver.PoseTasks();
    if (tasks.size() != 1 || tasks[0].first != kind || tasks[0].second != tool) { ++failures; std::printf("PoseTasks does not return what was set\n"); }
    const FirstOrderLoikOptimized::PoseResult r = solver.SolvePose({F}, 1.0, 1.0, 1e-6, 20, &q0);
    const std::vector<SE3> Fq = solver.FramePlacements(std::vector<Index>(1, ee), {tool});
    int reached = 0, free_moved = 0, unmasked = 0;
    const int off = what == 0 ? 3 : 0;   // where the masked-out half of err sits
    for (int b = 0; b < B; ++b) {
      reached += r.reached[b];
      for (int k = 0; k < 3; ++k) unmasked += r.err[(std::size_t)b * 6 + off + k] != 0.0;
      if (!r.reached[b]) continue;
      double dp = 0, dR = 0;
      for (int k = 0; k < 3; ++k) dp = std::fmax(dp, std::fabs(Fq[b][9 + k] - F[9 + k]));
      for (int k = 0; k < 9; ++k) dR = std::fmax(dR, std::fabs(Fq[b][k] - F[k]));
      // reached in the task's part (world-frame differences are the frame-axis ones up to a rotation: sqrt(3) covers it) ...
      if ((what == 0 ? dp : dR) > 2e-6) { ++failures; std::printf("instance %d reached but is %.3e off\n", b, what == 0 ? dp : dR); }
      // ... and the other part was left free
      free_moved += (what == 0 ? dR : dp) > 1e-4;
    }
    if (unmasked) { ++failures; std::printf("task %d: %d entries of err outside the mask are not zero\n", kind, unmasked); }
    if (reached < B * 9 / 10) { ++failures; std::printf("task %d: only %d of %d reached\n", kind, reached, B); }
    if (free_moved < reached / 2) { ++failures; std::printf("task %d: the free part matches the target on %d of %d\n", kind, reached - free_moved, reached); }
    std::printf("task %d: %d of %d reached, %d of them with the free part off the target\n", kind, reached, B, free_moved);
  }
  // bad arguments throw and leave the specification in place
  {
    SE3 bad = tool;
    bad[0] = 0.5;
    int n_threw = 0;
    try { solver.setPoseTasks({LOIKB_TASK_POSE}, {bad}); } catch (const std::runtime_error&) { ++n_threw; }
    try { solver.setPoseTasks({7}, {tool}); } catch (const std::runtime_error&) { ++n_threw; }
    try { solver.setPoseTasks({LOIKB_TASK_POSE, LOIKB_TASK_POSE}); } catch (const std::runtime_error&) { ++n_threw; }
    if (n_threw != 3) { ++failures; std::printf("%d of 3 bad task specifications threw\n", n_threw); }
    if (solver.PoseTasks().size() != 1) { ++failures; std::printf("a rejected specification changed the handle\n"); }
  }
  // an A written by the caller drops the specification; so does clearPoseTasks
  solver.UpdateEqConstraint(ee, Identity6(), std::vector<Vec6>{Vec6{}});
  if (!solver.PoseTasks().empty()) { ++failures; std::printf("UpdateEqConstraint with an A kept the tasks\n"); }
  solver.setPoseTasks({LOIKB_TASK_POSE});
  if (solver.PoseTasks().size() != 1) { ++failures; std::printf("setPoseTasks without frames failed\n"); }
  solver.clearPoseTasks();
  if (!solver.PoseTasks().empty()) { ++failures; std::printf("clearPoseTasks kept the tasks\n"); }
  if (failures) return 1;
  std::printf("all tasks checks passed\n");
  return 0;
}
