// Timed trajectories through the C++ mirror (include/loik_amd/loik.hpp: TrackPose; include/loik_amd_track.h): Talos-32, 6 instances,
// 4 steps along a smooth joint path each.  The mirror's result must be what the C ABI returns for the same call on a second handle,
// and the feed-forward must track better than pure feedback.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

int main()
{
  const Model model = Model::Builtin("talos32");
  const int B = 6, T = 4;
  const Index ee = (Index)loikb_builtin_joint_id("talos32", "arm_left_7_joint");
  IkIdDataOptimized data_a(model, 1, B), data_b(model, 1, B), data_c(model, 1, B);
  FirstOrderLoikOptimized a(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_a, true, 1e-1, false, false);
  FirstOrderLoikOptimized b(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_b, true, 1e-1, false, false);
  FirstOrderLoikOptimized c(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_c, true, 1e-1, false, false);
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  int failures = 0;
  // sample k of instance i: the end effector at q0_i + k * 0.01 * direction_i; instance i starts at q0_i, on its path
  auto config = [&](int i, double s) {
    DVec q(model.nq);
    for (int j = 0; j < model.nq; ++j) q[j] = 0.2 * std::sin(1.0 + i + 3.0 * j) + s * std::cos(2.0 + i + j);
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
  std::vector<SE3> smp((std::size_t)B * (T + 1));
  for (int k = 0; k <= T; ++k) {   // (FK of the path's configurations through handle c)
    for (int i = 0; i < B; ++i) {
      const DVec q = config(i, 0.01 * k);
      std::copy(q.begin(), q.end(), qw.begin() + (std::size_t)i * model.nq);
    }
    c.SolvePose(std::vector<SE3>(1, SE3{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}), 1.0, 1.0, 1e-6, 0, &qw);
    const std::vector<SE3> fk = c.ForwardKinematics({ee});
    for (int i = 0; i < B; ++i) smp[(std::size_t)i * (T + 1) + k] = fk[i];
  }
  bool threw = false;
  try { a.TrackPose(smp, 0); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("TrackPose with 0 steps did not throw\n"); }
  // the mirror against the C ABI on a second handle
  const FirstOrderLoikOptimized::TrackResult r = a.TrackPose(smp, T, 0.5, 1.0, 1e-3);
  DVec s12(smp.size() * 12);
  for (std::size_t i = 0; i < smp.size(); ++i) std::copy(smp[i].begin(), smp[i].end(), s12.begin() + 12 * i);
  const loikb_track_params p{0.5, 1.0, 1e-3, T, LOIKB_TRACK_FF_DIFFERENCE, LOIKB_TRACK_REC_Q | LOIKB_TRACK_REC_Z, 0};
  int rc = loikb_track_pose(b.handle(), nullptr, s12.data(), 0, &p);
  std::vector<int> inner((std::size_t)B * T), ontrack(B), worst_at(B);
  DVec qt((std::size_t)B * (T + 1) * model.nq), zt((std::size_t)B * T * model.nv), errmax((std::size_t)B * (T + 1)), worst(B);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_Q, qt.data(), 0);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_Z, zt.data(), 0);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_ERRMAX, errmax.data(), 0);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_INNER, inner.data(), 0);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_ONTRACK, ontrack.data(), 0);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_WORST, worst.data(), 0);
  if (!rc) rc = loikb_track_get(b.handle(), LOIKB_TRACK_F_WORST_AT, worst_at.data(), 0);
  if (rc) { ++failures; std::printf("the C ABI returned %d: %s\n", rc, loikb_last_error()); }
  if (r.q_traj != qt || r.z_traj != zt || r.errmax != errmax || r.worst != worst) { ++failures; std::printf("the mirror's q_traj / z_traj / errmax / worst differ from the C ABI's\n"); }
  if (r.inner != inner || r.ontrack != ontrack || r.worst_at != worst_at) { ++failures; std::printf("the mirror's inner / ontrack / worst_at differ from the C ABI's\n"); }
  if (a.q_resident() != b.q_resident()) { ++failures; std::printf("the resident q differs from the C ABI's\n"); }
  const DVec qa = a.q_resident();
  for (int i = 0; i < B; ++i) {
    if (r.steps[i] != T || (r.status[i] & (LOIKB_POSE_ST_REACHED | LOIKB_POSE_ST_STOPPED))) { ++failures; std::printf("instance %d: %d steps, status %d\n", i, r.steps[i], r.status[i]); }
    for (int j = 0; j < model.nq; ++j) {
      if (r.q_traj[((std::size_t)i * (T + 1)) * model.nq + j] != q0[(std::size_t)i * model.nq + j]) { ++failures; std::printf("q_traj[%d][0] is not the starting q\n", i); break; }
      if (r.q_traj[((std::size_t)i * (T + 1) + T) * model.nq + j] != qa[(std::size_t)i * model.nq + j]) { ++failures; std::printf("q_traj[%d][T] is not the final q\n", i); break; }
    }
  }
  // pure feedback lags by a sample: a larger worst error on every instance; without record there are no trajectories
  const FirstOrderLoikOptimized::TrackResult fb = a.TrackPose(smp, T, 0.5, 1.0, 1e-3, LOIKB_TRACK_FF_NONE, 0, &q0);
  int better = 0;
  for (int i = 0; i < B; ++i) better += r.worst[i] < fb.worst[i];
  if (better != B || !fb.q_traj.empty() || !fb.z_traj.empty()) { ++failures; std::printf("feed-forward better on %d of %d\n", better, B); }
  std::printf("feed-forward better on %d of %d, %d steps in the loop\n", better, B, (int)r.timing[0]);
  if (failures) return 1;
  std::printf("all track checks passed\n");
  return 0;
}
