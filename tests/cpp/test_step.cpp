// Step control through the C++ mirror (include/loik_amd/loik.hpp: setStepControl, clearStepControl, PoseResult::alpha / backtracks /
// failed; include/loik_amd_step.h): Panda-7, 32 instances 0.02 rad from their targets (the error
// is linear in the step there), gain 2.5, warm start off (so that a call does not depend on the calls before it).  The plain loop overshoots and
// diverges; with step control the batch reaches; with max_backtracks = 0 and patience = 3 every instance stalls after two moves,
// where a plain two-step solve leaves it; cleared, the handle runs the plain loop again, bit for bit.
// Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

int main()
{
  const Model model = Model::Builtin("panda7");
  const int B = 32;
  const Index ee = 7;
  const double gain = 2.5, tol = 1e-4;
  IkIdDataOptimized data(model, 1, B), data_c(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, false, 1e-1, false, false);
  FirstOrderLoikOptimized c(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_c, false, 1e-1, false, false);
  DVec q0((std::size_t)B * model.nq), qt((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) {
      q0[(std::size_t)b * model.nq + k] = 0.1 + 0.05 * std::sin(1.0 + b + 7.0 * k);
      qt[(std::size_t)b * model.nq + k] = q0[(std::size_t)b * model.nq + k] + 0.02 * std::cos(2.0 + b + k);
    }
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  int failures = 0;
  solver.SolveInit(q0, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  c.SolveInit(qt, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const std::vector<SE3> goal = c.ForwardKinematics({ee});
  auto count = [&](const std::vector<int>& v) { int n = 0; for (int x : v) n += x != 0; return n; };
  // bad parameters throw and change nothing
  const double bad_shrink[] = {0.0, 1.0, std::nan("")};
  for (double s : bad_shrink) {
    bool threw = false;
    try { solver.setStepControl(s); } catch (const std::runtime_error&) { threw = true; }
    if (!threw || loikb_pose_get_step_control(solver.handle(), nullptr)) { ++failures; std::printf("shrink %g did not throw, or left step control set\n", s); }
  }
  // the plain loop at this gain
  const FirstOrderLoikOptimized::PoseResult plain = solver.SolvePose(goal, 1.0, gain, tol, 30, &q0);
  if (!plain.alpha.empty()) { ++failures; std::printf("a plain solve returned alpha\n"); }
  const FirstOrderLoikOptimized::PoseResult two = solver.SolvePose(goal, 1.0, gain, tol, 2, &q0);
  const DVec q_two = solver.q_resident();
  // rescue
  solver.setStepControl();
  const FirstOrderLoikOptimized::PoseResult ctl = solver.SolvePose(goal, 1.0, gain, tol, 30, &q0);
  int backtracked = 0;
  for (int x : ctl.backtracks) backtracked += x > 0;
  std::printf("reached: plain %d, controlled %d of %d; %d instances backtracked\n", count(plain.reached), count(ctl.reached), B, backtracked);
  if (10 * count(plain.reached) > B) { ++failures; std::printf("the plain loop reaches more than 10 %%: the case shows nothing\n"); }
  if (10 * count(ctl.reached) < 9 * B) { ++failures; std::printf("the controlled loop reaches fewer than 90 %%\n"); }
  if (!backtracked || (int)ctl.alpha.size() != B || (int)ctl.failed.size() != B) { ++failures; std::printf("no backtrack recorded\n"); }
  for (int s : ctl.status)
    if (s & LOIKB_POSE_ST_STALLED) { ++failures; std::printf("STALLED with patience 0\n"); break; }
  // stall: no backtracking, patience 3
  solver.setStepControl(0.5, 1e-4, 0, 3);
  const FirstOrderLoikOptimized::PoseResult st = solver.SolvePose(goal, 1.0, gain, tol, 30, &q0);
  const DVec q_st = solver.q_resident();
  int stalled = 0;
  for (int b = 0; b < B; ++b) {
    if (!(st.status[b] & LOIKB_POSE_ST_STALLED)) continue;
    ++stalled;
    if (st.steps[b] != 2 || st.failed[b] != 3 || st.reached[b]) { ++failures; std::printf("instance %d stalled with steps %d failed %d\n", b, st.steps[b], st.failed[b]); break; }
  }
  if (stalled != B - count(plain.reached) || stalled == 0) { ++failures; std::printf("%d instances stalled, %d never reach in the plain loop\n", stalled, B - count(plain.reached)); }
  if (q_st != q_two) { ++failures; std::printf("the stalled q is not the plain loop's after two steps\n"); }
  if (st.err != two.err) { ++failures; std::printf("err of the stalled solve is not that of its final q\n"); }
  // cleared: the plain loop again
  solver.clearStepControl();
  const FirstOrderLoikOptimized::PoseResult again = solver.SolvePose(goal, 1.0, gain, tol, 2, &q0);
  if (again.steps != two.steps || again.status != two.status || again.err != two.err || solver.q_resident() != q_two || !again.alpha.empty()) {
    ++failures; std::printf("after clearing the solve differs from the plain one\n");
  }
  if (failures) return 1;
  std::printf("all step checks passed\n");
  return 0;
}
