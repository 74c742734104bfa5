// Waypoint paths through the C++ mirror (include/loik_amd/loik.hpp: SolvePosePath; include/loik_amd_path.h): Panda-7, 6 instances,
// 3 waypoints each.  The mirror's result must be what the C ABI returns for the same call on a second handle, one waypoint must
// be SolvePose, and a per-waypoint budget of 1 must stall.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

int main()
{
  const Model model = Model::Builtin("panda7");
  const int B = 6, T = 3;
  const Index ee = 7;
  IkIdDataOptimized data_a(model, 1, B), data_b(model, 1, B), data_c(model, 1, B);
  FirstOrderLoikOptimized a(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_a, true, 1e-1, false, false);
  FirstOrderLoikOptimized b(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_b, true, 1e-1, false, false);
  FirstOrderLoikOptimized c(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_c, true, 1e-1, false, false);
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  int failures = 0;
  // waypoint t of instance i: the end effector at q0 + (t + 1) * 0.05 * direction; instance i starts at q0_i
  auto config = [&](int i, double s) {
    DVec q(model.nq);
    for (int j = 0; j < model.nq; ++j) q[j] = (j == 3 ? -1.5 : 0.3) + 0.2 * std::sin(1.0 + i + 3.0 * j) + s * std::cos(2.0 + i + j);
    return q;
  };
  DVec q0((std::size_t)B * model.nq), qw((std::size_t)B * model.nq);
  for (int i = 0; i < B; ++i) {
    const DVec q = config(i, 0.0);
    std::copy(q.begin(), q.end(), q0.begin() + (std::size_t)i * model.nq);
  }
  a.SolveInit(q0, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  b.SolveInit(q0, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  c.SolveInit(q0, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  std::vector<SE3> wp((std::size_t)B * T);
  for (int t = 0; t < T; ++t) {   // (FK of the waypoint configurations through handle c, whose q is put back afterwards)
    for (int i = 0; i < B; ++i) {
      const DVec q = config(i, 0.05 * (t + 1));
      std::copy(q.begin(), q.end(), qw.begin() + (std::size_t)i * model.nq);
    }
    c.SolvePose(std::vector<SE3>(1, SE3{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}), 1.0, 1.0, 1e-6, 0, &qw);
    const std::vector<SE3> fk = c.ForwardKinematics({ee});
    for (int i = 0; i < B; ++i) wp[(std::size_t)i * T + t] = fk[i];
  }
  bool threw = false;
  try { a.SolvePosePath(wp, 0); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("SolvePosePath with 0 waypoints did not throw\n"); }
  // the mirror against the C ABI on a second handle
  const FirstOrderLoikOptimized::PathResult r = a.SolvePosePath(wp, T, 1.0, 1.0, 1e-5, 40);
  DVec w12(wp.size() * 12);
  for (std::size_t i = 0; i < wp.size(); ++i) std::copy(wp[i].begin(), wp[i].end(), w12.begin() + 12 * i);
  const loikb_pose_params p{1.0, 1.0, 1e-5, 40, 0};
  const loikb_path_params pp{T, 0, 1, 0};
  int rc = loikb_solve_pose_path(b.handle(), nullptr, w12.data(), 0, &p, &pp);
  std::vector<int> cursor(B), pstatus(B), wsteps((std::size_t)B * T);
  DVec qp((std::size_t)B * T * model.nq);
  if (!rc) rc = loikb_path_get(b.handle(), LOIKB_PATH_F_CURSOR, cursor.data(), 0);
  if (!rc) rc = loikb_path_get(b.handle(), LOIKB_PATH_F_STATUS, pstatus.data(), 0);
  if (!rc) rc = loikb_path_get(b.handle(), LOIKB_PATH_F_WSTEPS, wsteps.data(), 0);
  if (!rc) rc = loikb_path_get(b.handle(), LOIKB_PATH_F_Q, qp.data(), 0);
  if (rc) { ++failures; std::printf("the C ABI returned %d: %s\n", rc, loikb_last_error()); }
  if (r.cursor != cursor || r.path_status != pstatus || r.wsteps != wsteps) { ++failures; std::printf("the mirror's cursor / status / wsteps differ from the C ABI's\n"); }
  int complete = 0, nan_rows = 0;
  for (int i = 0; i < B; ++i) {
    complete += r.path_status[i] == LOIKB_PATH_ST_COMPLETE && r.cursor[i] == T && r.reached[i];
    int total = 0;
    for (int t = 0; t < T; ++t) total += r.wsteps[(std::size_t)i * T + t];
    if (total != r.steps[i]) { ++failures; std::printf("instance %d: wsteps do not add up to steps\n", i); }
    for (int t = 0; t < T; ++t)
      for (int j = 0; j < model.nq; ++j) {
        const double x = r.q_path[((std::size_t)i * T + t) * model.nq + j], y = qp[((std::size_t)i * T + t) * model.nq + j];
        nan_rows += std::isnan(x);
        if (!(x == y) && !(std::isnan(x) && std::isnan(y))) { ++failures; std::printf("q_path differs from the C ABI's\n"); }
      }
  }
  if (complete < B - 1) { ++failures; std::printf("only %d of %d paths complete\n", complete, B); }
  if (complete == B && nan_rows) { ++failures; std::printf("NaN rows in a complete result\n"); }
  // one waypoint is SolvePose
  std::vector<SE3> last(B);
  for (int i = 0; i < B; ++i) last[i] = wp[(std::size_t)i * T + T - 1];
  const FirstOrderLoikOptimized::PathResult one = a.SolvePosePath(last, 1, 1.0, 1.0, 1e-5, 3, 0, true, &q0);
  const DVec qa = a.q_resident();
  const FirstOrderLoikOptimized::PoseResult ps = b.SolvePose(last, 1.0, 1.0, 1e-5, 3, &q0);
  if (one.steps != ps.steps || one.status != ps.status || one.err != ps.err || qa != b.q_resident()) { ++failures; std::printf("one waypoint is not SolvePose\n"); }
  // a budget of one step per waypoint stalls, without record there is no q_path
  const FirstOrderLoikOptimized::PathResult st = a.SolvePosePath(wp, T, 1.0, 0.5, 1e-9, 40, 1, false, &q0);
  int stalled = 0;
  for (int i = 0; i < B; ++i) stalled += st.path_status[i] == LOIKB_PATH_ST_STALLED && !st.reached[i] && st.steps[i] == st.cursor[i] + 1;
  if (stalled != B || !st.q_path.empty()) { ++failures; std::printf("%d of %d stalled with a budget of 1\n", stalled, B); }
  std::printf("%d of %d paths complete, %d steps in the loop\n", complete, B, (int)r.timing[0]);
  if (failures) return 1;
  std::printf("all path checks passed\n");
  return 0;
}
