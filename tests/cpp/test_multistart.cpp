// Multi-start pose IK through the C++ mirror (include/loik_amd/loik.hpp: setSeedRanges, SampleSeeds, SolvePoseMultiStart;
// include/loik_amd_multistart.h): Panda-7, 4 goals with 8 seeds each.  The mirror's winner and q must be what the C ABI returns
// for the same call on a second handle.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

int main()
{
  const Model model = Model::Builtin("panda7");
  const int G = 4, K = 8, B = G * K;
  const Index ee = 7;
  IkIdDataOptimized data_a(model, 1, B), data_b(model, 1, B);
  FirstOrderLoikOptimized a(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_a, true, 1e-1, false, false);
  FirstOrderLoikOptimized b(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data_b, true, 1e-1, false, false);
  // ranges of our own (these handles carry no joint limits), the same for every joint but the fourth (whose range is negative)
  DVec lo(model.nv, -1.0), hi(model.nv, 1.0), w(model.nv, 1.0), mid(model.nq, 0.0);
  lo[3] = -2.5; hi[3] = -0.5; mid[3] = -1.5; w[0] = 3.0;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  int failures = 0;
  bool threw = false;
  try { a.SampleSeeds(K, 1, 0, &mid); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("SampleSeeds before SolveInit did not throw\n"); }
  // the goals: the end effector at four configurations inside the ranges
  DVec qg((std::size_t)B * model.nq);
  for (int g = 0; g < G; ++g)
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < model.nq; ++j) qg[((std::size_t)g * K + k) * model.nq + j] = mid[j] + 0.4 * std::sin(1.0 + g + 3.0 * j);
  a.SolveInit(qg, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  b.SolveInit(qg, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const std::vector<SE3> fk = a.ForwardKinematics({ee});
  std::vector<SE3> targets;
  for (int g = 0; g < G; ++g) targets.push_back(fk[(std::size_t)g * K]);
  threw = false;
  try { a.SolvePoseMultiStart(targets, K, 2, 5); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("SolvePoseMultiStart without ranges or limits did not throw\n"); }
  a.setSeedRanges(lo, hi, w);
  // SampleSeeds: seed 0 of round 0 is q0, every other coordinate is inside its range; round 1 differs
  a.SampleSeeds(K, 5, 0, &mid);
  const DVec s0 = a.q_resident();
  a.SampleSeeds(K, 5, 1, &mid);
  const DVec s1 = a.q_resident();
  int outside = 0, same = 0;
  for (int i = 0; i < B; ++i)
    for (int j = 0; j < model.nq; ++j) {
      const double x = s0[(std::size_t)i * model.nq + j];
      if (i % K == 0 && x != mid[j]) { ++failures; std::printf("seed 0 of goal %d is not q0\n", i / K); }
      outside += x < lo[j] || x > hi[j];
      same += i % K != 0 && x == s1[(std::size_t)i * model.nq + j];
    }
  if (outside || same) { ++failures; std::printf("%d samples outside their range, %d equal in rounds 0 and 1\n", outside, same); }
  // the mirror against the C ABI on a second handle
  const FirstOrderLoikOptimized::MultiStartResult r = a.SolvePoseMultiStart(targets, K, 2, 5, LOIKB_MS_PICK_NEAREST, &mid, 1.0, 1.0, 1e-6, 30);
  DVec t12((std::size_t)G * 12);
  for (int g = 0; g < G; ++g) std::copy(targets[g].begin(), targets[g].end(), t12.begin() + 12 * g);
  const loikb_pose_params p{1.0, 1.0, 1e-6, 30, 0};
  const loikb_multistart_params m{K, 2, 5ull, LOIKB_MS_PICK_NEAREST, 0};
  int rc = loikb_multistart_set_ranges(b.handle(), lo.data(), hi.data(), w.data(), model.nv);
  if (!rc) rc = loikb_solve_pose_multistart(b.handle(), mid.data(), t12.data(), LOIKB_Q_SHARED, &p, &m);
  std::vector<int> winner(G), status(G);
  DVec q((std::size_t)G * model.nq);
  if (!rc) rc = loikb_multistart_get(b.handle(), LOIKB_MS_F_WINNER, winner.data(), 0);
  if (!rc) rc = loikb_multistart_get(b.handle(), LOIKB_MS_F_GOAL_STATUS, status.data(), 0);
  if (!rc) rc = loikb_multistart_get(b.handle(), LOIKB_MS_F_Q, q.data(), 0);
  if (rc) { ++failures; std::printf("the C ABI returned %d: %s\n", rc, loikb_last_error()); }
  if (r.winner != winner || r.goal_status != status || r.q != q) { ++failures; std::printf("the mirror's winner / status / q differ from the C ABI's\n"); }
  int reached = 0;
  for (int g = 0; g < G; ++g) {
    reached += r.goal_status[g] == LOIKB_MS_GOAL_REACHED;
    if (r.winner[g] / K != g) { ++failures; std::printf("goal %d: winner %d is not one of its instances\n", g, r.winner[g]); }
  }
  if (reached < G - 1) { ++failures; std::printf("only %d of %d goals reached\n", reached, G); }
  if (r.rounds_run < 1 || r.rounds_run > 2 || (int)r.round.size() != B) { ++failures; std::printf("rounds_run %d\n", r.rounds_run); }
  std::printf("%d of %d goals reached in %d round(s)\n", reached, G, r.rounds_run);
  if (failures) return 1;
  std::printf("all multistart checks passed\n");
  return 0;
}
