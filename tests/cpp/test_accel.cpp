// Joint acceleration limits through the C++ mirror (include/loik_amd/loik.hpp: setJointAccelLimits, clearJointAccelLimits,
// setStartVelocity, AppliedVelocity; include/loik_amd_accel.h): Panda-7, 32 instances tracking a target that jumps away from them.
// The recorded velocities obey |z_k - z_{k-1}| <= a dt, the applied velocity is the last row and round-trips through the C ABI,
// a chained call continues where the first ended, and the same run without the limits breaks the bound.
// Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

int main()
{
  const Model model = Model::Builtin("panda7");
  const int B = 32, T = 4;
  const Index ee = 7;
  const double inf = std::numeric_limits<double>::infinity(), dt = 0.5, a = 0.05;
  IkIdDataOptimized data(model, 1, B), data_c(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, false, 1e-1, false, false);
  FirstOrderLoikOptimized c(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_c, false, 1e-1, false, false);
  DVec q0((std::size_t)B * model.nq), qt((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) {
      q0[(std::size_t)b * model.nq + k] = 0.1 + 0.05 * std::sin(1.0 + b + 7.0 * k);
      qt[(std::size_t)b * model.nq + k] = q0[(std::size_t)b * model.nq + k] + 0.2 * std::cos(2.0 + b + k);
    }
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  int failures = 0;
  solver.SolveInit(q0, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  c.SolveInit(qt, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const std::vector<SE3> goal = c.ForwardKinematics({ee});   // a constant target 0.2 away in joint space: the samples of every step
  std::vector<SE3> smp((std::size_t)B * (2 * T + 1));
  for (int b = 0; b < B; ++b)
    for (int k = 0; k <= 2 * T; ++k) smp[(std::size_t)b * (2 * T + 1) + k] = goal[b];
  auto part = [&](int from, int n) {   // samples from .. from + n of every instance
    std::vector<SE3> s((std::size_t)B * (n + 1));
    for (int b = 0; b < B; ++b)
      for (int k = 0; k <= n; ++k) s[(std::size_t)b * (n + 1) + k] = smp[(std::size_t)b * (2 * T + 1) + from + k];
    return s;
  };
  // bad limits throw; the getter throws before a loop with limits
  for (int what = 0; what < 3; ++what) {
    DVec bad(model.nv + (what == 0), 1.0);
    if (what == 1) bad[2] = std::nan("");
    if (what == 2) bad[2] = 0.0;
    bool threw = false;
    try { solver.setJointAccelLimits(bad); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { ++failures; std::printf("bad acceleration limits (%d) did not throw\n", what); }
  }
  bool threw = false;
  try { (void)solver.AppliedVelocity(); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("AppliedVelocity before a loop with limits did not throw\n"); }
  DVec a_max(model.nv, a);
  a_max[1] = inf;   // one DoF without a limit
  auto worst_jump = [&](const DVec& z, int steps, const DVec* start) {   // max over limited DoFs of |z_k - z_{k-1}| / (a dt), z_{-1} = start or 0
    double w = 0.0;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < steps; ++k)
        for (int j = 0; j < model.nv; ++j) {
          if (j == 1) continue;
          const double prev = k ? z[((std::size_t)b * steps + k - 1) * model.nv + j] : (start ? (*start)[(std::size_t)b * model.nv + j] : 0.0);
          w = std::fmax(w, std::fabs(z[((std::size_t)b * steps + k) * model.nv + j] - prev) / (a * dt));
        }
    return w;
  };
  // without the limits the jump is taken at once
  const FirstOrderLoikOptimized::TrackResult free_run = solver.TrackPose(smp, 2 * T, dt, 1.0, 1e-3, LOIKB_TRACK_FF_NONE);
  const double free_jump = worst_jump(free_run.z_traj, 2 * T, nullptr);
  if (!(free_jump > 2.0)) { ++failures; std::printf("without limits the worst jump is only %.3f a dt: the case shows nothing\n", free_jump); }
  // with them every step obeys the bound, and the INNER bit says so
  solver.setJointAccelLimits(a_max);
  const FirstOrderLoikOptimized::TrackResult whole = solver.TrackPose(smp, 2 * T, dt, 1.0, 1e-3, LOIKB_TRACK_FF_NONE, LOIKB_TRACK_REC_Q | LOIKB_TRACK_REC_Z, &q0);
  const double lim_jump = worst_jump(whole.z_traj, 2 * T, nullptr);
  if (!(lim_jump <= 1.0 + 1e-12)) { ++failures; std::printf("with limits the worst jump is %.17g a dt\n", lim_jump); }
  int accel_bits = 0;
  for (int v : whole.inner) accel_bits += (v & 8) != 0;
  if (!accel_bits) { ++failures; std::printf("INNER never carries the acceleration bit\n"); }
  const std::vector<int> flags = solver.PoseLimitFlags();
  int accel_flags = 0;
  for (int f : flags) {
    accel_flags += (f & (LOIKB_LIMIT_ACCEL_LOWER | LOIKB_LIMIT_ACCEL_UPPER)) != 0;
    if (f & (LOIKB_LIMIT_LOWER | LOIKB_LIMIT_UPPER)) { ++failures; std::printf("a position flag without position limits\n"); break; }
  }
  if (!accel_flags) { ++failures; std::printf("no acceleration flag in the limit flags\n"); }
  // the applied velocity is the last row of z, and what the C ABI returns
  const DVec v_end = solver.AppliedVelocity();
  DVec v_abi((std::size_t)B * model.nv);
  if (loikb_accel_get_velocity(solver.handle(), v_abi.data(), 0) != 0 || v_abi != v_end) { ++failures; std::printf("AppliedVelocity differs from the C ABI's\n"); }
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < model.nv; ++j)
      if (v_end[(std::size_t)b * model.nv + j] != whole.z_traj[((std::size_t)b * 2 * T + 2 * T - 1) * model.nv + j]) { ++failures; std::printf("AppliedVelocity is not the last z\n"); b = B; break; }
  // two chained calls are the one call (warm_start off): the second starts from the first's applied velocity
  const FirstOrderLoikOptimized::TrackResult first = solver.TrackPose(part(0, T), T, dt, 1.0, 1e-3, LOIKB_TRACK_FF_NONE, LOIKB_TRACK_REC_Q | LOIKB_TRACK_REC_Z, &q0);
  const DVec v_mid = solver.AppliedVelocity();
  solver.setStartVelocity(v_mid);
  const FirstOrderLoikOptimized::TrackResult second = solver.TrackPose(part(T, T), T, dt, 1.0, 1e-3, LOIKB_TRACK_FF_NONE);
  for (int b = 0; b < B && !failures; ++b)
    for (int k = 0; k < T; ++k)
      for (int j = 0; j < model.nv; ++j) {
        if (first.z_traj[((std::size_t)b * T + k) * model.nv + j] != whole.z_traj[((std::size_t)b * 2 * T + k) * model.nv + j] ||
            second.z_traj[((std::size_t)b * T + k) * model.nv + j] != whole.z_traj[((std::size_t)b * 2 * T + T + k) * model.nv + j]) {
          ++failures; std::printf("chained calls differ from the one call at instance %d step %d DoF %d\n", b, k, j); b = B; k = T; break;
        }
      }
  if (!(worst_jump(second.z_traj, T, &v_mid) <= 1.0 + 1e-12)) { ++failures; std::printf("the seam breaks the bound\n"); }
  // cleared: as if never set
  solver.clearJointAccelLimits();
  const FirstOrderLoikOptimized::TrackResult again = solver.TrackPose(smp, 2 * T, dt, 1.0, 1e-3, LOIKB_TRACK_FF_NONE, LOIKB_TRACK_REC_Q | LOIKB_TRACK_REC_Z, &q0);
  if (again.z_traj != free_run.z_traj || again.q_traj != free_run.q_traj) { ++failures; std::printf("after clearing the run differs from the one before the limits\n"); }
  threw = false;
  try { (void)solver.AppliedVelocity(); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("AppliedVelocity after a loop without limits did not throw\n"); }
  std::printf("worst jump %.3f a dt without limits, %.15f with; %d steps flagged\n", free_jump, lim_jump, accel_bits);
  if (failures) return 1;
  std::printf("all accel checks passed\n");
  return 0;
}
