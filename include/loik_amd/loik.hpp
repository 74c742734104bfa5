// loik_amd/loik.hpp -- C++17 host-side mirror of the reference's solver interface over the C-ABI (loik_amd.h).
//
// Same class / method names, argument order and error behaviour as
//   loik::FirstOrderLoikOptimizedTpl<double>   (/root/reference/include/loik/loik-loid-optimized.hpp:22-808)
//   loik::IkIdDataTypeOptimizedTpl<double>     (/root/reference/include/loik/loik-loid-data-optimized.hpp:62-379)
//   loik::IkIdSolverBaseTpl<double>            (/root/reference/include/loik/task-solver-base.hpp:21-174)
// so a caller of the reference switches by changing the namespace and the vector types (no Eigen / Pinocchio in
// this image: 6-vectors are std::array<double,6> in Pinocchio's [linear; angular] order, 6x6 matrices are row-major
// std::array<double,36>; INTEGRATION.md shows the two-line Eigen/Pinocchio adapters).
//
// The one addition is the batch: `batch` independent problem instances are solved by one object on one MI355X.
// With batch == 1 every call has exactly the reference's single-instance meaning.  For batch > 1 the per-instance
// inputs are instance-major arrays (q[batch*nq], bis[batch*nc], ...); results land in the caller-owned data
// object, as upstream (the solver keeps `IkIdData&`, loik-loid-optimized.hpp:763).
// All compute happens in libloik_amd.so on the GPU; there is no CPU path behind this header.
#pragma once

#include "../loik_amd.h"
#include "../loik_amd_pose.h"
#include "../loik_amd_limits.h"
#include "../loik_amd_tasks.h"
#include "../loik_amd_multistart.h"
#include "../loik_amd_path.h"
#include "../loik_amd_track.h"
#include "../loik_amd_accel.h"
#include "../loik_amd_step.h"
#include "../loik_amd_axis.h"
#include "../loik_amd_jacobian.h"
#include "../loik_amd_collision.h"
#include "../loik_amd_motion.h"
#include "../loik_amd_avoid.h"
#include "../loik_amd_shortcut.h"
#include "../loik_amd_retime.h"
#include "../loik_amd_blend.h"
#include "../loik_amd_plan.h"
#include "../loik_amd_grid.h"
#include "../loik_amd_gridnear.h"
#include "../loik_amd_depth.h"

#include <array>
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

namespace loik_amd {

// task-solver-base.hpp:13-18
enum ADMMPenaltyUpdateStrat { DEFAULT = 0, OSQP = 1, MAXEIGENVALUE = 3 };

using Index = std::size_t;
using DVec = std::vector<double>;
using Vec6 = std::array<double, 6>;
using Mat6x6 = std::array<double, 36>;  // row-major
using Motion = Vec6;                    // [linear; angular]

inline Mat6x6 Identity6()
{
  Mat6x6 m{};
  for (int k = 0; k < 6; ++k) m[7 * k] = 1.0;
  return m;
}

// the members of pinocchio::Model the hot path reads (loik-loid-optimized.hxx:46-47, :118-119, :257-265)
struct Model {
  int njoints = 0, nq = 0, nv = 0;
  std::vector<int> parents, jtype, idx_q, idx_v;
  std::vector<double> axis;             // [njoints][3]
  std::vector<double> jointPlacements;  // [njoints][12]: R row-major, t
  std::vector<std::string> names;
  // JointModelComposite (empty when the model has none): joint i of type LOIKB_J_COMPOSITE = sub-joints comp_first[i] ..
  // comp_first[i] + comp_count[i] - 1 of comp_jtype / comp_axis / comp_placement (include/loik_amd_models.h)
  std::vector<int> comp_first, comp_count, comp_jtype;
  std::vector<double> comp_axis, comp_placement;
  std::vector<double> comp_pitch;  // [n_sub] the same for helical sub-joints of composites (empty: none)
  std::vector<double> pitch;  // [njoints] JointModelHelical*::m_pitch (LOIKB_J_HX .. HU); empty when the model has no helical joint

  static Model Builtin(const std::string& name)
  {
    loikb_model_desc d{};
    if (loikb_builtin_model(name.c_str(), &d, nullptr, nullptr) != 0) throw std::runtime_error("unknown built-in model " + name);
    Model m;
    m.njoints = d.njoints; m.nq = d.nq; m.nv = d.nv;
    m.parents.assign(d.parents, d.parents + d.njoints);
    m.jtype.assign(d.jtype, d.jtype + d.njoints);
    m.idx_q.assign(d.idx_q, d.idx_q + d.njoints);
    m.idx_v.assign(d.idx_v, d.idx_v + d.njoints);
    m.axis.assign(d.axis, d.axis + 3 * d.njoints);
    m.jointPlacements.assign(d.placement, d.placement + 12 * d.njoints);
    for (int i = 0; i < d.njoints; ++i) m.names.emplace_back(loikb_builtin_joint_name(name.c_str(), i));
    return m;
  }
  Index getJointId(const std::string& n) const
  {
    for (std::size_t i = 0; i < names.size(); ++i)
      if (names[i] == n) return i;
    return names.size();
  }
  loikb_model_desc desc() const
  {
    loikb_model_desc d{};
    d.njoints = njoints; d.nq = nq; d.nv = nv;
    d.parents = parents.data(); d.jtype = jtype.data(); d.axis = axis.data();
    d.idx_q = idx_q.data(); d.idx_v = idx_v.data(); d.placement = jointPlacements.data();
    if (!comp_jtype.empty()) {
      d.comp_first = comp_first.data(); d.comp_count = comp_count.data(); d.comp_jtype = comp_jtype.data();
      d.comp_axis = comp_axis.data(); d.comp_placement = comp_placement.data();
    }
    if (!pitch.empty()) d.pitch = pitch.data();
    if (!comp_pitch.empty()) d.comp_pitch = comp_pitch.data();
    return d;
  }
};

class FirstOrderLoikOptimized;

// LoikSolverInfo of the reference (loik-loid-optimized.hpp:47-127; base lists task-solver-base.hpp:25-52): the lists a solver
// constructed with logging = true fills, for one instance.  Upstream keeps the struct protected; get_solver_info() hands it out.
struct LoikSolverInfo {
  std::vector<int> iter_list_, tail_solve_iter_list_;
  std::vector<double> primal_residual_task_list_, primal_residual_slack_list_, primal_residual_list_, dual_residual_nu_list_,
      dual_residual_v_list_, dual_residual_list_, mu_list_, mu_eq_list_, mu_ineq_list_;
  int Size() const { return (int)iter_list_.size(); }
};

// A member of the data object that is fetched from the device the first time it is read after a solve (His, pis, Aty,
// liMi: large, rarely read -- upstream's tests read His / pis, tests/loik-loid.cpp:597-615).  Reads like the std::vector it
// wraps: operator[], data(), size(), begin()/end(), implicit conversion to const DVec&.
class LazyField {
public:
  LazyField() = default;
  LazyField(int field, std::size_t n) : field_(field), buf_(n, 0.0) {}
  const DVec& get() const;
  operator const DVec&() const { return get(); }
  double operator[](std::size_t i) const { return get()[i]; }
  const double* data() const { return get().data(); }
  std::size_t size() const { return buf_.size(); }
  DVec::const_iterator begin() const { return get().begin(); }
  DVec::const_iterator end() const { return get().end(); }

private:
  friend class FirstOrderLoikOptimized;
  friend struct IkIdDataOptimized;
  int field_ = -1;
  mutable DVec buf_;
  mutable unsigned long long seen_ = 0;                  // generation of the solver state the buffer holds
  const FirstOrderLoikOptimized* owner_ = nullptr;       // set by the solver that references the data object
  const unsigned long long* generation_ = nullptr;
};

// caller-owned result / state object (public members, as upstream).  Instance b, joint i (1..nb), component k:
//   z[b*nv + j], nu[...], w[...];  vis[(b*nb + (i-1))*6 + k], fis likewise;  yis[(b*nc + c)*6 + k], Aty likewise;
//   His[(b*nb + (i-1))*21 + sym(r,c)] (upper triangle, row-major: H_i is symmetric);  pis like vis;
//   liMi[(b*nb + (i-1))*12 + ..] = R row-major, t.
// z, nu, w, vis, fis, yis are copied after every solve (selectable: FirstOrderLoikOptimized::set_fetch); His, pis, Aty, liMi
// are fetched on first access.
struct IkIdDataOptimized {
  IkIdDataOptimized(const Model& model, int num_eq_c_, int batch_ = 1)
  : batch(batch_), nb(model.njoints - 1), nv(model.nv), num_eq_c(num_eq_c_),
    nu(static_cast<std::size_t>(batch_) * model.nv, 0.0), z(nu.size(), 0.0), w(nu.size(), 0.0),
    vis(static_cast<std::size_t>(batch_) * (model.njoints - 1) * 6, 0.0), fis(vis.size(), 0.0),
    yis(static_cast<std::size_t>(batch_) * num_eq_c_ * 6, 0.0),
    His(LOIKB_F_HIS, static_cast<std::size_t>(batch_) * (model.njoints - 1) * 21),
    pis(LOIKB_F_PIS, static_cast<std::size_t>(batch_) * (model.njoints - 1) * 6),
    Aty(LOIKB_F_ATY, static_cast<std::size_t>(batch_) * num_eq_c_ * 6),
    liMi(LOIKB_F_LIMI, static_cast<std::size_t>(batch_) * (model.njoints - 1) * 12)
  {
  }
  int batch, nb, nv, num_eq_c;
  DVec nu, z, w;  // z is the answer: box-projected joint velocity (loik-loid-optimized.hpp:333)
  DVec vis, fis, yis;
  LazyField His, pis, Aty, liMi;
  // full symmetric 6x6 of link i (1..nb) of instance b out of the packed His
  Mat6x6 His_full(int i, int b = 0) const
  {
    const DVec& h = His.get();
    const double* p = h.data() + (static_cast<std::size_t>(b) * nb + (i - 1)) * 21;
    Mat6x6 m{};
    int k = 0;
    for (int r = 0; r < 6; ++r)
      for (int c = r; c < 6; ++c, ++k) { m[6 * r + c] = p[k]; m[6 * c + r] = p[k]; }
    return m;
  }
};

// ---- what IntegrateDepth and IntegratePoints of FirstOrderLoikOptimized take and return (include/loik_amd_depth.h)
// DepthCamera: a pinhole camera; T_world_cam = (R row-major, p) places its frame (x right, y down, z forward) in the world
struct DepthCamera {
  int width = 0, height = 0;
  double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;
  std::array<double, 12> T_world_cam{{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}};
  double depth_scale = 1.0, z_min = 0.0, z_max = 0.0;
};
struct DepthStats {
  long long returns = 0, inside = 0, occupied_before = 0, occupied_after = 0;
};
// what both calls take beside the sensor's data: fuse = onto the occupancy of the grid that is set (else the frame alone), carve (fuse
// and a camera only) = less the voxels the frame sees through by more than band; filter_q [n][nq] = configurations whose collision
// spheres, padded by filter_pad, are cut out; filter_resident > 0 (with an empty filter_q) = the first so many resident configurations.
// band and filter_pad < 0: (sqrt(3) / 2) voxel, what the header says they must at least cover
struct DepthOptions {
  bool fuse = false, carve = false;
  double band = -1.0, filter_pad = -1.0;
  DVec filter_q;
  int filter_resident = 0;
};

class FirstOrderLoikOptimized {
public:
  using IkIdData = IkIdDataOptimized;

  // the reference's 17 constructor arguments, same order (loik-loid-optimized.hpp:129-134), then batch / device
  FirstOrderLoikOptimized(const int max_iter, const double& tol_abs, const double& tol_rel, const double& tol_primal_inf,
                          const double& tol_dual_inf, const double& rho, const double& mu,
                          const double& mu_equality_scale_factor, const ADMMPenaltyUpdateStrat& mu_update_strat,
                          const int num_eq_c, const int eq_c_dim, const Model& model, IkIdData& ik_id_data,
                          const bool warm_start, const double tol_tail_solve, const bool verbose, const bool logging,
                          const int device = 0, const int flags = 0, const int eq_c_capacity = 0)
  : model_(model), ik_id_data_(ik_id_data), batch_(ik_id_data.batch), nc_(num_eq_c)
  {
    loikb_options o{};
    o.max_iter = max_iter; o.tol_abs = tol_abs; o.tol_rel = tol_rel; o.tol_primal_inf = tol_primal_inf;
    o.tol_dual_inf = tol_dual_inf; o.rho = rho; o.mu = mu; o.mu_equality_scale_factor = mu_equality_scale_factor;
    o.mu_update_strat = mu_update_strat; o.num_eq_c = num_eq_c; o.eq_c_dim = eq_c_dim; o.warm_start = warm_start;
    o.tol_tail_solve = tol_tail_solve; o.verbose = verbose; o.logging = logging;
    o.batch = batch_; o.device = device; o.precision = LOIKB_F64; o.flags = flags;
    o.eq_c_capacity = eq_c_capacity;  // room for AddEqConstraint (0: num_eq_c slots, as upstream sizes yis / Aty)
    const loikb_model_desc d = model_.desc();
    if (loikb_version() != LOIKB_VERSION)  // (struct layouts of this header against the loaded library's)
      throw std::runtime_error("loik_amd: libloik_amd.so has ABI version " + std::to_string(loikb_version()) + ", this header is version " +
                               std::to_string(LOIKB_VERSION) + ": rebuild the library");
    check(loikb_create(&d, &o, &h_));
    max_iter_ = max_iter; rho_ = rho; tol_tail_solve_ = tol_tail_solve; tol_primal_inf_ = tol_primal_inf; tol_dual_inf_ = tol_dual_inf;
    for (LazyField* f : {&ik_id_data_.His, &ik_id_data_.pis, &ik_id_data_.Aty, &ik_id_data_.liMi}) {
      f->owner_ = this;
      f->generation_ = &generation_;
    }
  }
  ~FirstOrderLoikOptimized() { loikb_destroy(h_); }
  FirstOrderLoikOptimized(const FirstOrderLoikOptimized&) = delete;
  FirstOrderLoikOptimized& operator=(const FirstOrderLoikOptimized&) = delete;

  // loik-loid-optimized.hpp:335-361
  void SolveInit(const DVec& q, const Mat6x6& H_ref, const Motion& v_ref, const std::vector<Index>& active_task_constraint_ids,
                 const std::vector<Mat6x6>& Ais, const std::vector<Vec6>& bis, const DVec& lb, const DVec& ub)
  {
    Args a(*this, q, active_task_constraint_ids, Ais, bis, lb, ub);
    check(loikb_solve_init(h_, q.data(), H_ref.data(), v_ref.data(), a.ids.data(), (int)a.ids.size(), a.A.data(),
                           a.b.data(), lb.data(), ub.data(), a.nbound, a.flags));
  }
  // loik-loid-optimized.hpp:368-455
  void Solve()
  {
    check(loikb_solve(h_));
    solved();
  }
  // loik-loid-optimized.hpp:475-580
  void Solve(const DVec& q, const Mat6x6& H_ref, const Motion& v_ref, const std::vector<Index>& active_task_constraint_ids,
             const std::vector<Mat6x6>& Ais, const std::vector<Vec6>& bis, const DVec& lb, const DVec& ub)
  {
    Args a(*this, q, active_task_constraint_ids, Ais, bis, lb, ub);
    check(loikb_solve_full(h_, q.data(), H_ref.data(), v_ref.data(), a.ids.data(), (int)a.ids.size(), a.A.data(),
                           a.b.data(), lb.data(), ub.data(), a.nbound, a.flags));
    solved();
  }
  // loik-loid-optimized.hpp:596-695 (one Ai for the batch; bi per instance when bi.size() == batch)
  void Solve(const DVec& q, const Index c_id, const Mat6x6& Ai, const Vec6& bi)
  {
    int flags = LOIKB_A_SHARED | LOIKB_B_SHARED;
    check_q(q);
    if (batch_ > 1 && q.size() == static_cast<std::size_t>(model_.nq)) flags |= LOIKB_Q_SHARED;
    check(loikb_solve_tailored(h_, q.data(), (int)c_id, Ai.data(), bi.data(), flags));
    solved();
  }
  void Solve(const DVec& q, const Index c_id, const Mat6x6& Ai, const std::vector<Vec6>& bis)
  {
    DVec b(bis.size() * 6);
    for (std::size_t i = 0; i < bis.size(); ++i)
      for (int k = 0; k < 6; ++k) b[6 * i + k] = bis[i][k];
    int flags = LOIKB_A_SHARED;
    check_bis(bis);
    if (bis.size() == 1 && batch_ > 1) flags |= LOIKB_B_SHARED;
    check_q(q);
    if (batch_ > 1 && q.size() == static_cast<std::size_t>(model_.nq)) flags |= LOIKB_Q_SHARED;
    check(loikb_solve_tailored(h_, q.data(), (int)c_id, Ai.data(), b.data(), flags));
    solved();
  }

  // ---- IkProblemFormulationOptimized's editing methods (ik-id-description-optimized.hpp).  Upstream they sit behind the
  // protected problem_ member (loik-loid-optimized.hpp:765): a subclass reaches them; here they are public.  They act on the
  // problem the last SolveInit / Solve(q, H_ref, ...) set and stay in force until the next one.
  // UpdateReferences(H_refs, v_refs), :103-121: one weight and target per joint, index 0 = the universe
  void UpdateReferences(const std::vector<Mat6x6>& H_refs, const std::vector<Motion>& v_refs)
  {
    if (H_refs.size() != v_refs.size() || H_refs.size() != static_cast<std::size_t>(model_.njoints))
      throw std::runtime_error("[IkProblemFormulation::UpdateReferences]: input arguments 'H_refs', 'v_refs' have wrong size!!");
    DVec H(H_refs.size() * 36), v(v_refs.size() * 6);
    for (std::size_t i = 0; i < H_refs.size(); ++i) {
      for (int k = 0; k < 36; ++k) H[36 * i + k] = H_refs[i][k];
      for (int k = 0; k < 6; ++k) v[6 * i + k] = v_refs[i][k];
    }
    check(loikb_update_references(h_, H.data(), v.data(), (int)H_refs.size()));
  }
  // UpdateEqConstraint(c_id, Ai, bi) :178-218 and (c_id, bi) :224-238; bis: one per instance or one for the batch
  void UpdateEqConstraint(const Index c_id, const Mat6x6& Ai, const std::vector<Vec6>& bis)
  {
    const DVec b = flat(bis);
    check(loikb_update_eq_constraint(h_, (int)c_id, Ai.data(), b.data(), LOIKB_A_SHARED | b_flag(bis)));
  }
  void UpdateEqConstraint(const Index c_id, const std::vector<Vec6>& bis)
  {
    const DVec b = flat(bis);
    check(loikb_update_eq_constraint(h_, (int)c_id, nullptr, b.data(), b_flag(bis)));
  }
  // AddEqConstraint, :244-286 (needs a free slot: constructor argument eq_c_capacity)
  void AddEqConstraint(const Index c_id, const Mat6x6& Ai, const std::vector<Vec6>& bis)
  {
    const DVec b = flat(bis);
    check(loikb_add_eq_constraint(h_, (int)c_id, Ai.data(), b.data(), LOIKB_A_SHARED | b_flag(bis)));
    resize_constraints();
  }
  // RemoveEqConstraint, :292-319; false: nothing to remove (upstream prints a warning)
  bool RemoveEqConstraint(const Index c_id)
  {
    const int rc = loikb_remove_eq_constraint(h_, (int)c_id);
    if (rc < 0) check(rc);
    resize_constraints();
    return rc == LOIKB_OK;
  }
  std::vector<Index> active_task_constraint_ids() const
  {
    std::vector<int> ids(static_cast<std::size_t>(loikb_eq_c_capacity(h_)) + 1);
    const int n = loikb_active_constraint_ids(h_, ids.data(), (int)ids.size());
    return std::vector<Index>(ids.begin(), ids.begin() + n);
  }
  // solve on the edited set without rewriting a constraint (not upstream, whose tailored Solve always updates one)
  void Solve(const DVec& q)
  {
    int flags = 0;
    check_q(q);
    if (batch_ > 1 && q.size() == static_cast<std::size_t>(model_.nq)) flags |= LOIKB_Q_SHARED;
    check(loikb_solve_tailored(h_, q.data(), -1, nullptr, nullptr, flags));
    solved();
  }

  // ---- pass-level public methods (loik-loid-optimized.hpp:192-264; the reference's component-wise test calls them one by one,
  // tests/loik-loid.cpp:305-556).  They run on the plain one-instance-per-thread implementation behind loikb_pass (a debug
  // path; the Solve() overloads use the fused kernels); after each call the data object is refreshed like after a solve.
  void FwdPass1() { pass(LOIKB_PASS_FWD_PASS1); }
  void BwdPassOptimizedVisitor() { pass(LOIKB_PASS_BWD_PASS); }
  void FwdPass2OptimizedVisitor() { pass(LOIKB_PASS_FWD_PASS2); }
  void BoxProj() { pass(LOIKB_PASS_BOX_PROJ); }
  void DualUpdate() { pass(LOIKB_PASS_DUAL_UPDATE); }
  void ComputeResiduals() { pass(LOIKB_PASS_COMPUTE_RESIDUALS); }
  void CheckConvergence() { pass(LOIKB_PASS_CHECK_CONVERGENCE); }
  void CheckFeasibility() { pass(LOIKB_PASS_CHECK_FEASIBILITY); }
  void UpdateMu() { pass(LOIKB_PASS_UPDATE_MU); }
  // iter_ = i; ik_id_data_.UpdatePrev(); ik_id_data_.ResetInfNorms()  -- the head of a loop iteration (hpp:381-388)
  void BeginIteration() { pass(LOIKB_PASS_BEGIN_ITERATION); }

  // ---- outer loop on the device (not in the reference class: its callers -- a sampling planner, README.md:5 --
  //      integrate on the host and pass a new q to the tailored Solve every step; here q stays resident in HBM)
  // q <- q (+) dt * z, z = the answer of the last solve
  void Integrate(double dt) { check(loikb_integrate(h_, dt)); }
  // tailored Solve (loik-loid-optimized.hpp:596-695) on the resident q
  void Solve(const Index c_id, const Mat6x6& Ai, const std::vector<Vec6>& bis)
  {
    DVec b(bis.size() * 6);
    for (std::size_t i = 0; i < bis.size(); ++i)
      for (int k = 0; k < 6; ++k) b[6 * i + k] = bis[i][k];
    int flags = LOIKB_A_SHARED;
    check_bis(bis);
    if (bis.size() == 1 && batch_ > 1) flags |= LOIKB_B_SHARED;
    check(loikb_solve_tailored(h_, nullptr, (int)c_id, Ai.data(), b.data(), flags));
    solved();
  }
  // ---- batched pose IK (include/loik_amd_pose.h): per step e_c = log6(oMi_c^-1 oMdes_c), b_c = A_c (gain / dt) e_c, the tailored
  //      Solve on the resident q, q <- q (+) dt z for the instances not yet reached.  A placement is R row-major, then t.
  using SE3 = std::array<double, 12>;
  struct PoseResult {
    std::vector<int> reached, steps, status;  // [batch]; status: LOIKB_POSE_ST_* bits
    DVec err;                                 // [batch][nc][6]: e_c of the final q, [linear; angular]
    // with step control set (setStepControl), else empty: alpha of the last step that moved the instance (0: none), the sum of the
    // accepted trial numbers, the searches that accepted no trial; LOIKB_POSE_ST_STALLED is a bit of `status`
    DVec alpha;
    std::vector<int> backtracks, failed;
  };
  // targets: one per active constraint (active_task_constraint_ids order) for the whole batch, or batch * nc instance-major;
  // q: nullptr = the resident configurations, else [batch][nq] replaces them first
  PoseResult SolvePose(const std::vector<SE3>& targets, double dt = 1.0, double gain = 1.0, double tol_pose = 1e-6, int max_steps = 100,
                       const DVec* q = nullptr)
  {
    const std::size_t nc = (std::size_t)loikb_num_eq_c(h_);
    int flags = 0;
    if (targets.size() == nc && batch_ > 1) flags |= LOIKB_POSE_TARGET_SHARED;
    else if (targets.size() != (std::size_t)batch_ * nc)
      throw std::runtime_error("loik_amd: SolvePose needs one target per active constraint, shared or per instance");
    if (q && q->size() != (std::size_t)batch_ * model_.nq) throw std::runtime_error("loik_amd: q must hold batch * model.nq values");
    DVec t(targets.size() * 12);
    for (std::size_t i = 0; i < targets.size(); ++i) std::copy(targets[i].begin(), targets[i].end(), t.begin() + 12 * i);
    const loikb_pose_params p{dt, gain, tol_pose, max_steps, 0};
    check(loikb_solve_pose(h_, q ? q->data() : nullptr, t.data(), flags, &p));
    solved();
    PoseResult r;
    r.steps.resize(batch_); r.status.resize(batch_); r.reached.resize(batch_); r.err.resize((std::size_t)batch_ * nc * 6);
    check(loikb_pose_get(h_, LOIKB_POSE_F_STEPS, r.steps.data(), 0));
    check(loikb_pose_get(h_, LOIKB_POSE_F_STATUS, r.status.data(), 0));
    check(loikb_pose_get(h_, LOIKB_POSE_F_ERR, r.err.data(), 0));
    for (int b = 0; b < batch_; ++b) r.reached[b] = (r.status[b] & LOIKB_POSE_ST_REACHED) ? 1 : 0;
    if (loikb_pose_get_step_control(h_, nullptr)) {
      r.alpha.resize(batch_); r.backtracks.resize(batch_); r.failed.resize(batch_);
      check(loikb_step_get(h_, LOIKB_STEP_F_ALPHA, r.alpha.data(), 0));
      check(loikb_step_get(h_, LOIKB_STEP_F_BACKTRACKS, r.backtracks.data(), 0));
      check(loikb_step_get(h_, LOIKB_STEP_F_FAILED, r.failed.data(), 0));
    }
    return r;
  }
  // world placements oMi of `links` for the resident q: [batch][links.size()]
  std::vector<SE3> ForwardKinematics(const std::vector<Index>& links) const
  {
    std::vector<int> l(links.begin(), links.end());
    DVec out((std::size_t)batch_ * l.size() * 12);
    check(loikb_forward_kinematics(h_, l.data(), (int)l.size(), out.data(), 0));
    std::vector<SE3> M((std::size_t)batch_ * l.size());
    for (std::size_t i = 0; i < M.size(); ++i) std::copy(out.begin() + 12 * i, out.begin() + 12 * (i + 1), M[i].begin());
    return M;
  }
  // ---- joint position limits of the pose loop, the velocity-box update (include/loik_amd_limits.h)
  // q_lo, q_hi: [nv], -inf / +inf = no limit on that side; honoured by every later SolvePose.  clearJointLimits(): as if never set.
  void setJointLimits(const DVec& q_lo, const DVec& q_hi)
  {
    if (q_lo.size() != q_hi.size()) throw std::runtime_error("loik_amd: q_lo and q_hi differ in size");
    check(loikb_set_joint_limits(h_, q_lo.data(), q_hi.data(), (int)q_lo.size()));
  }
  void clearJointLimits() { check(loikb_set_joint_limits(h_, nullptr, nullptr, 0)); }
  // UpdateIneqConstraints(lb, ub) of the problem formulation (ik-id-description-optimized.hpp:325-339): [nv] = one box for the batch,
  // [batch][nv] = one per instance; any other size is the library's LOIKB_ERR_INEQ_DIM
  void UpdateIneqConstraints(const DVec& lb, const DVec& ub)
  {
    if (lb.size() != ub.size()) throw std::runtime_error("loik_amd: lb and ub differ in size");
    const bool per_inst = batch_ > 1 && lb.size() == (std::size_t)batch_ * model_.nv;
    check(loikb_update_ineq_constraints(h_, lb.data(), ub.data(), per_inst ? model_.nv : (int)lb.size(), per_inst ? 0 : LOIKB_BOUNDS_SHARED));
  }
  // [batch][nv] LOIKB_LIMIT_LOWER / LOIKB_LIMIT_UPPER bits of the last SolvePose with limits (throws when it ran without)
  std::vector<int> PoseLimitFlags() const
  {
    std::vector<int> f((std::size_t)batch_ * model_.nv);
    check(loikb_pose_get_limit_flags(h_, f.data(), 0));
    return f;
  }
  // ---- joint acceleration limits of the pose loops, braking-aware position limits (include/loik_amd_accel.h)
  // a_max: [nv], entries > 0, +inf = no limit on that DoF; honoured by every later SolvePose / SolvePosePath / TrackPose.
  // clearJointAccelLimits(): as if never set.
  void setJointAccelLimits(const DVec& a_max) { check(loikb_set_joint_accel_limits(h_, a_max.data(), (int)a_max.size())); }
  void clearJointAccelLimits() { check(loikb_set_joint_accel_limits(h_, nullptr, 0)); }
  // v0: [batch][nv], the velocity the next pose loop starts from (then forgotten); empty = rest
  void setStartVelocity(const DVec& v0)
  {
    if (!v0.empty() && v0.size() != (std::size_t)batch_ * model_.nv) throw std::runtime_error("loik_amd: v0 needs batch * nv entries");
    check(loikb_accel_set_start_velocity(h_, v0.empty() ? nullptr : v0.data(), 0));
  }
  // [batch][nv] the velocity applied in the last step that moved each instance of the last pose loop with acceleration limits (0: never
  // moved, reached or stopped; throws when it ran without)
  DVec AppliedVelocity() const
  {
    DVec v((std::size_t)batch_ * model_.nv);
    check(loikb_accel_get_velocity(h_, v.data(), 0));
    return v;
  }
  // ---- backtracking step control and stall detection of SolvePose (include/loik_amd_step.h)
  // per step the trials q (+) alpha dt z, alpha = 1, shrink, shrink^2, ... (max_backtracks + 1 of them); the first that brings the
  // squared pose error down to (1 - sufficient alpha) of its value is taken, the plain step if none; patience > 0: an instance whose
  // searches failed that many times in a row is LOIKB_POSE_ST_STALLED and left where it was.  clearStepControl(): as if never set.
  void setStepControl(double shrink = 0.5, double sufficient = 1e-4, int max_backtracks = 6, int patience = 0)
  {
    const loikb_step_params p{shrink, sufficient, max_backtracks, patience, 0};
    check(loikb_pose_set_step_control(h_, &p));
  }
  void clearStepControl() { check(loikb_pose_set_step_control(h_, nullptr)); }
  // ---- tool frames and position-only / orientation-only tasks of the pose loop (include/loik_amd_tasks.h)
  // kinds: LOIKB_TASK_POSE / _POSITION / _ORIENTATION, or with the rotation about the frame's z axis free LOIKB_TASK_POSE_AXIS / _AXIS
  // (include/loik_amd_axis.h), one per active constraint (active_task_constraint_ids order); frames: iMf of
  // the task frame on the constrained link, one per kind, or empty = the joint frame.  A formulation edit: every active constraint's
  // A becomes the shared A_c = S_c X_c^-1 and its b zero.  clearPoseTasks(): the specification goes, A stays.
  void setPoseTasks(const std::vector<int>& kinds, const std::vector<SE3>& frames = {})
  {
    if (!frames.empty() && frames.size() != kinds.size()) throw std::runtime_error("loik_amd: kinds and frames differ in size");
    DVec f(frames.size() * 12);
    for (std::size_t i = 0; i < frames.size(); ++i) std::copy(frames[i].begin(), frames[i].end(), f.begin() + 12 * i);
    check(loikb_pose_set_tasks(h_, (int)kinds.size(), kinds.data(), frames.empty() ? nullptr : f.data()));
  }
  void clearPoseTasks() { check(loikb_pose_clear_tasks(h_)); }
  // the tasks in force: (kind, iMf) per active constraint; empty when there are none
  std::vector<std::pair<int, SE3>> PoseTasks() const
  {
    const int n = loikb_pose_get_tasks(h_, nullptr, nullptr, 0);
    std::vector<int> k((std::size_t)std::max(n, 0));
    DVec f(k.size() * 12);
    if (n > 0) (void)loikb_pose_get_tasks(h_, k.data(), f.data(), n);
    std::vector<std::pair<int, SE3>> out(k.size());
    for (std::size_t i = 0; i < out.size(); ++i) {
      out[i].first = k[i];
      std::copy(f.begin() + 12 * i, f.begin() + 12 * (i + 1), out[i].second.begin());
    }
    return out;
  }
  // world placements oMf = oMi(links[e]) * frames[e] for the resident q: [batch][links.size()]; frames empty = ForwardKinematics
  std::vector<SE3> FramePlacements(const std::vector<Index>& links, const std::vector<SE3>& frames = {}) const
  {
    if (!frames.empty() && frames.size() != links.size()) throw std::runtime_error("loik_amd: links and frames differ in size");
    std::vector<int> l(links.begin(), links.end());
    DVec f(frames.size() * 12), out((std::size_t)batch_ * l.size() * 12);
    for (std::size_t i = 0; i < frames.size(); ++i) std::copy(frames[i].begin(), frames[i].end(), f.begin() + 12 * i);
    check(loikb_frame_placements(h_, l.data(), frames.empty() ? nullptr : f.data(), (int)l.size(), out.data(), 0));
    std::vector<SE3> M((std::size_t)batch_ * l.size());
    for (std::size_t i = 0; i < M.size(); ++i) std::copy(out.begin() + 12 * i, out.begin() + 12 * (i + 1), M[i].begin());
    return M;
  }
  // ---- frame Jacobians and dexterity of the resident q (include/loik_amd_jacobian.h)
  // J [batch][links.size()][6][nv] with v_f = J nu, v_f = [linear; angular] of the frame oMi(links[e]) * frames[e] (frames empty =
  // the joint frames), in LOIKB_JAC_LOCAL / _LOCAL_WORLD_ALIGNED / _WORLD
  DVec FrameJacobians(const std::vector<Index>& links, const std::vector<SE3>& frames = {}, int reference_frame = LOIKB_JAC_LOCAL) const
  {
    if (!frames.empty() && frames.size() != links.size()) throw std::runtime_error("loik_amd: links and frames differ in size");
    if (links.empty()) return {};
    std::vector<int> l(links.begin(), links.end());
    DVec f(frames.size() * 12), out((std::size_t)batch_ * l.size() * 6 * model_.nv);
    for (std::size_t i = 0; i < frames.size(); ++i) std::copy(frames[i].begin(), frames[i].end(), f.begin() + 12 * i);
    check(loikb_frame_jacobians(h_, l.data(), frames.empty() ? nullptr : f.data(), (int)l.size(), reference_frame, out.data(), 0));
    return out;
  }
  // [batch][n][LOIKB_DEX_N]: sigma_0 .. sigma_5 (descending, 0 past the selected rows), manipulability, inverse condition number of
  // diag(1/length x 3, 1 x 3) S_rows J_local.  rows: 6-bit masks, empty = all six rows.  TaskDexterity(length): the same for the handle's
  // tasks -- the active constraint links with the frames and rows of setPoseTasks (identity, all six rows without tasks)
  DVec FrameDexterity(const std::vector<Index>& links, const std::vector<SE3>& frames = {}, const std::vector<int>& rows = {},
                      double length = 1.0) const
  {
    if ((!frames.empty() && frames.size() != links.size()) || (!rows.empty() && rows.size() != links.size()))
      throw std::runtime_error("loik_amd: links, frames and rows differ in size");
    if (links.empty()) return {};
    std::vector<int> l(links.begin(), links.end());
    DVec f(frames.size() * 12), out((std::size_t)batch_ * l.size() * LOIKB_DEX_N);
    for (std::size_t i = 0; i < frames.size(); ++i) std::copy(frames[i].begin(), frames[i].end(), f.begin() + 12 * i);
    const loikb_dexterity_params p{length, 0};
    check(loikb_frame_dexterity(h_, l.data(), frames.empty() ? nullptr : f.data(), rows.empty() ? nullptr : rows.data(), (int)l.size(), &p,
                                out.data(), 0));
    return out;
  }
  DVec TaskDexterity(double length = 1.0) const
  {
    const int nc = loikb_num_eq_c(h_);
    if (nc <= 0) return {};
    DVec out((std::size_t)batch_ * (std::size_t)nc * LOIKB_DEX_N);
    const loikb_dexterity_params p{length, 0};
    check(loikb_frame_dexterity(h_, nullptr, nullptr, nullptr, nc, &p, out.data(), 0));
    return out;
  }
  // the dexterous pick of SolvePoseMultiStart: among the reached seeds of a goal, the one whose worst task has the largest smallest
  // singular value (cost = -min_c sigma_min of TaskDexterity(length)); clear: as if never set.  Returns the length, 0 when not set
  void setMultiStartPickDexterous(double length = 1.0)
  {
    const loikb_dexterity_params p{length, 0};
    check(loikb_dexterity_set_multistart_pick(h_, &p));
  }
  void clearMultiStartPickDexterous() { check(loikb_dexterity_set_multistart_pick(h_, nullptr)); }
  double MultiStartPickDexterous() const
  {
    loikb_dexterity_params p{0.0, 0};
    return loikb_dexterity_get_multistart_pick(h_, &p) ? p.length : 0.0;
  }
  // ---- collision clearance (include/loik_amd_collision.h): a sphere model of the robot against a world of spheres and oriented boxes and
  // against itself.  spheres [ns][4] = (x, y, z, r) in the frame of links[s] (0 = the universe); empty clears the spheres and the self pairs
  void setCollisionSpheres(const std::vector<Index>& links, const DVec& spheres)
  {
    if (spheres.size() != 4 * links.size()) throw std::runtime_error("loik_amd: need four numbers per sphere");
    std::vector<int> l(links.begin(), links.end());
    check(loikb_collision_set_spheres(h_, l.data(), spheres.data(), (int)l.size()));
    nspheres_ = l.size();
  }
  // world spheres [nws][4] = (x, y, z, r) and oriented boxes [nwb][15] = (R row-major, p, half extents); both empty clears the world
  void setCollisionWorld(const DVec& wspheres = {}, const DVec& wboxes = {})
  {
    if (wspheres.size() % 4 != 0 || wboxes.size() % 15 != 0) throw std::runtime_error("loik_amd: need 4 numbers per world sphere, 15 per box");
    check(loikb_collision_set_world(h_, wspheres.data(), (int)(wspheres.size() / 4), wboxes.data(), (int)(wboxes.size() / 15)));
  }
  // the sphere pairs (a < b) whose links differ, are not parent and child and are not in `ignore` (link pairs, either order)
  void setSelfCollision(bool enable = true, const std::vector<std::array<Index, 2>>& ignore = {})
  {
    std::vector<int> ig;
    for (const auto& pr : ignore) { ig.push_back((int)pr[0]); ig.push_back((int)pr[1]); }
    check(loikb_collision_set_self_pairs(h_, enable ? 1 : 0, ig.data(), (int)ignore.size()));
  }
  int NumSelfPairs() const { return loikb_collision_num_self_pairs(h_); }
  struct ClearanceResult {
    DVec min, min_world, min_self;   // [n]; +inf over an empty set of pairs, NaN for a q that is not finite
    std::vector<int> witness;        // [n][3] = (LOIKB_CLR_* kind, robot sphere, obstacle or other sphere) of the pair that achieves min
  };
  // of the resident q of the batch (q = nullptr), or of any number of configurations q [n][nq]
  ClearanceResult Clearance(const DVec* q = nullptr) const
  {
    const std::size_t n = q ? q->size() / (std::size_t)model_.nq : (std::size_t)batch_;
    if (q && q->size() != n * (std::size_t)model_.nq) throw std::runtime_error("loik_amd: q is not a whole number of configurations");
    DVec m(3 * n);
    ClearanceResult r;
    r.witness.resize(3 * n);
    check(loikb_clearance(h_, q ? q->data() : nullptr, (int)n, 0, m.data(), r.witness.data(), 0));
    r.min.resize(n); r.min_world.resize(n); r.min_self.resize(n);
    for (std::size_t i = 0; i < n; ++i) { r.min[i] = m[3 * i]; r.min_world[i] = m[3 * i + 1]; r.min_self[i] = m[3 * i + 2]; }
    return r;
  }
  // the collision-aware SolvePoseMultiStart: a goal is answered only by a reached seed whose clearance is >= margin; clear: as if never
  // set.  MultiStartClearance(&margin) returns whether it is set
  void setMultiStartClearance(double margin = 0.0)
  {
    const loikb_clearance_params p{margin, 0};
    check(loikb_clearance_set_multistart(h_, &p));
  }
  void clearMultiStartClearance() { check(loikb_clearance_set_multistart(h_, nullptr)); }
  bool MultiStartClearance(double* margin = nullptr) const
  {
    loikb_clearance_params p{0.0, 0};
    if (!loikb_clearance_get_multistart(h_, &p)) return false;
    if (margin) *margin = p.margin;
    return true;
  }
  // ---- voxel worlds (include/loik_amd_grid.h): an occupancy grid as one more world object beside the spheres and boxes.  occupancy
  // [nz][ny][nx] (nonzero = occupied), dims = (nx, ny, nz), origin the low corner of voxel (0, 0, 0), voxel the edge.  The distance field
  // is built on the device before the call returns; Clearance, the collision-aware multi-start and the motion layer read it.
  // ClearCollisionGrid: as if never set
  void SetCollisionGrid(const std::vector<unsigned char>& occupancy, const std::array<int, 3>& dims, const std::array<double, 3>& origin, double voxel)
  {
    if (occupancy.empty() || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 ||
        occupancy.size() != (std::size_t)dims[0] * (std::size_t)dims[1] * (std::size_t)dims[2])
      throw std::runtime_error("loik_amd: need nx * ny * nz > 0 occupancy bytes");
    check(loikb_collision_set_world_grid(h_, occupancy.data(), dims.data(), origin.data(), voxel, 0));
  }
  void ClearCollisionGrid() { check(loikb_collision_set_world_grid(h_, nullptr, nullptr, nullptr, 0.0, 0)); }
  struct CollisionGrid {
    std::array<int, 3> dims{{0, 0, 0}};          // nx, ny, nz
    std::array<double, 3> origin{{0.0, 0.0, 0.0}};
    double voxel = 0.0;
    std::vector<unsigned int> G;                 // [nz][ny][nx]: (voxel / 2) sqrt(G) is the distance of a voxel's centre to the occupied cubes,
                                                 // LOIKB_GRID_EMPTY where nothing is occupied; empty with field = false
  };
  // whether a grid is set; with out, what was set and (field = true) the distance field
  bool GetCollisionGrid(CollisionGrid* out = nullptr, bool field = true) const
  {
    CollisionGrid g;
    const int rc = loikb_collision_get_world_grid(h_, g.dims.data(), g.origin.data(), &g.voxel, nullptr, 0);
    if (rc < 0) check(rc);
    if (rc == 0) return false;
    if (out) {
      if (field) {
        g.G.resize((std::size_t)g.dims[0] * (std::size_t)g.dims[1] * (std::size_t)g.dims[2]);
        const int rc2 = loikb_collision_get_world_grid(h_, nullptr, nullptr, nullptr, g.G.data(), 0);
        if (rc2 < 0) check(rc2);
      }
      *out = std::move(g);
    }
    return true;
  }
  // ---- the nearest-voxel transform (include/loik_amd_gridnear.h): with the latch on every grid that is set gets its transform F beside
  // the field, and collision avoidance reads the grid as one more world object of every sphere
  void SetCollisionGridNearest(bool on = true) { check(loikb_collision_grid_set_nearest(h_, on ? 1 : 0)); }
  // whether the latch is on and a grid is set; with out, F [nz][ny][nx]: the occupied voxel nearest to each voxel
  bool GetCollisionGridNearest(std::vector<unsigned int>* out = nullptr) const
  {
    const int rc = loikb_collision_grid_get_nearest(h_, nullptr, 0);
    if (rc < 0) check(rc);
    if (rc == 0) return false;
    if (out) {
      CollisionGrid g;
      GetCollisionGrid(&g, false);
      out->resize((std::size_t)g.dims[0] * (std::size_t)g.dims[1] * (std::size_t)g.dims[2]);
      const int rc2 = loikb_collision_grid_get_nearest(h_, out->data(), 0);
      if (rc2 < 0) check(rc2);
    }
    return true;
  }
  struct GridNearestResult {
    DVec val;              // [n][2]: the lower bound v of the grid header, d_u - r with d_u the distance to the chosen cube
    std::vector<int> vox;  // [n][2]: the voxel read, the chosen cube (-1 in an empty grid)
    DVec normal;           // [n][3]: the outward normal of the chosen cube
  };
  // the grid pair with a direction of spheres [n][4] = x y z r in the world frame
  GridNearestResult GridNearest(const DVec& spheres) const
  {
    const std::size_t n = spheres.size() / 4;
    if (spheres.size() != 4 * n) throw std::runtime_error("loik_amd: spheres is not a whole number of (x, y, z, r) rows");
    GridNearestResult r;
    r.val.resize(2 * n); r.vox.resize(2 * n); r.normal.resize(3 * n);
    check(loikb_grid_nearest_query(h_, spheres.data(), (int)n, 0, r.val.data(), r.vox.data(), r.normal.data(), 0));
    return r;
  }
  // ---- depth images and point clouds (include/loik_amd_depth.h): the voxel world from what a sensor delivers, integrated on the device.
  using DepthCamera = loik_amd::DepthCamera;
  using DepthStats = loik_amd::DepthStats;
  using DepthOptions = loik_amd::DepthOptions;
  // depth [height][width] row-major, float metres (times depth_scale)
  DepthStats IntegrateDepth(const std::vector<float>& depth, const DepthCamera& cam, const std::array<int, 3>& dims, const std::array<double, 3>& origin,
                            double voxel, const DepthOptions& opt = DepthOptions())
  {
    return integrate_depth_(depth.data(), depth.size(), LOIKB_DEPTH_F32, cam, dims, origin, voxel, opt);
  }
  // ... or unsigned 16-bit image units (times depth_scale)
  DepthStats IntegrateDepth(const std::vector<unsigned short>& depth, const DepthCamera& cam, const std::array<int, 3>& dims, const std::array<double, 3>& origin,
                            double voxel, const DepthOptions& opt = DepthOptions())
  {
    return integrate_depth_(depth.data(), depth.size(), LOIKB_DEPTH_U16, cam, dims, origin, voxel, opt);
  }
  // points [n][3] in the world frame; nothing is carved
  DepthStats IntegratePoints(const DVec& points, const std::array<int, 3>& dims, const std::array<double, 3>& origin, double voxel, const DepthOptions& opt = DepthOptions())
  {
    const std::size_t n = points.size() / 3;
    if (points.size() != 3 * n) throw std::runtime_error("loik_amd: points is not a whole number of (x, y, z) rows");
    int nf = 0;
    const loikb_depth_params prm = depth_params_(opt, voxel, &nf);
    long long st[4] = {0, 0, 0, 0};
    check(loikb_collision_grid_integrate_points(h_, points.data(), (int)n, dims.data(), origin.data(), voxel, &prm, opt.filter_q.empty() ? nullptr : opt.filter_q.data(),
                                                nf, 0, st));
    return DepthStats{st[0], st[1], st[2], st[3]};
  }
  // whether a grid is set; with out, its occupancy [nz][ny][nx] as 0 / 1 bytes, whichever call set it
  bool GetCollisionOccupancy(std::vector<unsigned char>* out = nullptr) const
  {
    const int rc = loikb_collision_grid_get_occupancy(h_, nullptr, 0);
    if (rc < 0) check(rc);
    if (rc == 0) return false;
    if (out) {
      CollisionGrid g;
      GetCollisionGrid(&g, false);
      out->resize((std::size_t)g.dims[0] * (std::size_t)g.dims[1] * (std::size_t)g.dims[2]);
      const int rc2 = loikb_collision_grid_get_occupancy(h_, out->data(), 0);
      if (rc2 < 0) check(rc2);
    }
    return true;
  }
  // ---- motions (include/loik_amd_motion.h).  Difference: v [n][nv] with q0 (+) v = q1 under Integrate's arithmetic
  DVec Difference(const DVec& q0, const DVec& q1) const
  {
    const std::size_t n = q0.size() / (std::size_t)model_.nq;
    if (q0.size() != q1.size() || q0.size() != n * (std::size_t)model_.nq) throw std::runtime_error("loik_amd: q0 and q1 are not the same whole number of configurations");
    DVec v(n * (std::size_t)model_.nv);
    check(loikb_difference(h_, q0.data(), q1.data(), (int)n, 0, v.data(), 0));
    return v;
  }
  struct MotionResult {
    std::vector<int> status, evals;     // [n]; status: LOIKB_MOTION_*
    DVec s_free, min_sampled, s_at_min; // [n]
    std::vector<int> witness;           // [n][3] of min_sampled, as ClearanceResult::witness
  };
  // the certified check of the segments q(s) = qa (+) s dv, s in [0, 1]: qa [n][nq], dv [n][nv]
  MotionResult MotionClearance(const DVec& qa, const DVec& dv, double margin = 0.0, double tol = 1e-3, int max_evals = 256) const
  {
    const std::size_t n = qa.size() / (std::size_t)model_.nq;
    if (qa.size() != n * (std::size_t)model_.nq || dv.size() != n * (std::size_t)model_.nv) throw std::runtime_error("loik_amd: qa and dv are not the same whole number of rows");
    const loikb_motion_params p{margin, tol, max_evals, 0};
    DVec val(3 * n);
    std::vector<int> info(5 * n);
    check(loikb_motion_clearance(h_, qa.data(), dv.data(), (int)n, 0, &p, val.data(), info.data(), 0));
    return motion_result(val, info);
  }
  // ... of every segment between consecutive samples of q_path [B][T][nq]: the result has B (T - 1) rows, path major
  MotionResult PathClearance(const DVec& q_path, int T, double margin = 0.0, double tol = 1e-3, int max_evals = 256) const
  {
    const std::size_t per = (std::size_t)(T > 0 ? T : 1) * (std::size_t)model_.nq, B = q_path.size() / per;
    if (q_path.size() != B * per) throw std::runtime_error("loik_amd: q_path is not a whole number of paths of T samples");
    const loikb_motion_params p{margin, tol, max_evals, 0};
    const std::size_t n = B * (std::size_t)(T > 1 ? T - 1 : 0);
    DVec val(3 * n);
    std::vector<int> info(5 * n);
    check(loikb_motion_clearance_path(h_, q_path.data(), (int)B, T, 0, &p, val.data(), info.data(), 0));
    return motion_result(val, info);
  }
  // ---- shortcutting (include/loik_amd_shortcut.h).  ShortcutPaths: per path of q_path [B][T][nq] `rounds` draws of a sub-path whose
  // straight joint-space segment replaces it when the check of MotionClearance certifies the segment FREE.  n_waypoints [B]: the leading
  // rows of each path that are waypoints (empty: T everywhere)
  struct ShortcutResult {
    DVec q_path;                         // [B][T][nq]: the kept waypoints, the last one repeated
    std::vector<int> n_waypoints, keep;  // [B]; [B][T] input row indices, -1 after the kept ones
    std::vector<int> tried, accepted, blocked, undecided, invalid;   // [B]
    DVec length_in, length_out;          // [B], as PathLength
  };
  ShortcutResult ShortcutPaths(const DVec& q_path, int T, const std::vector<int>& n_waypoints = {}, int rounds = 64, unsigned long long seed = 0,
                               double margin = 0.0, double tol = 1e-3, int max_evals = 256) const
  {
    const std::size_t B = path_count(q_path, T, n_waypoints);
    const loikb_shortcut_params p{margin, tol, max_evals, rounds, seed, 0};
    ShortcutResult r;
    r.q_path.resize(q_path.size());
    r.keep.resize(B * (std::size_t)(T > 0 ? T : 0));
    std::vector<int> info(6 * B);
    DVec val(2 * B);
    check(loikb_shortcut_paths(h_, q_path.data(), n_waypoints.empty() ? nullptr : n_waypoints.data(), (int)B, T, 0, &p, r.q_path.data(), r.keep.data(),
                               info.data(), val.data(), 0));
    split_info(info, 6, {&r.n_waypoints, &r.tried, &r.accepted, &r.blocked, &r.undecided, &r.invalid});
    split_info(val, 2, {&r.length_in, &r.length_out});
    return r;
  }
  // the joint-space length [B] of the paths: the sum over consecutive waypoints of the norm of their Difference
  DVec PathLength(const DVec& q_path, int T, const std::vector<int>& n_waypoints = {}) const
  {
    const std::size_t B = path_count(q_path, T, n_waypoints);
    DVec length(B);
    check(loikb_path_length(h_, q_path.data(), n_waypoints.empty() ? nullptr : n_waypoints.data(), (int)B, T, 0, length.data(), 0));
    return length;
  }
  // ---- retiming (include/loik_amd_retime.h).  RetimePaths: the paths q_path [B][T][nq] as samples q(t), v(t) at the period dt under the
  // per-DoF limits v_max, a_max [nv], every segment from rest to rest on a trapezoid of its path parameter; every sample lies on a segment
  // of the input.  max_samples = the rows S of the result; < 0 sizes S to the largest n_samples with a timing-only call first, 0 is a
  // timing-only call.  snap stretches every segment to whole samples (LOIKB_RETIME_SNAP)
  struct RetimeResult {
    int S = 0;                                            // rows of q_traj / v_traj per path
    DVec q_traj, v_traj;                                  // [B][S][nq], [B][S][nv]
    std::vector<int> n_samples, n_waypoints, moved, flags;   // [B]; flags: LOIKB_RETIME_TRUNCATED / INVALID / SKIPPED
    DVec duration, seg;                                   // [B]; [B][T-1][4] = (t_start, duration, t_acc, peak)
  };
  RetimeResult RetimePaths(const DVec& q_path, int T, const DVec& v_max, const DVec& a_max, double dt, const std::vector<int>& n_waypoints = {},
                           int max_samples = -1, bool snap = false) const
  {
    const std::size_t B = path_count(q_path, T, n_waypoints);
    const loikb_retime_params p{dt, snap ? LOIKB_RETIME_SNAP : 0};
    const int* len = n_waypoints.empty() ? nullptr : n_waypoints.data();
    RetimeResult r;
    r.duration.resize(B);
    r.seg.resize(4 * B * (std::size_t)(T > 1 ? T - 1 : 0));
    std::vector<int> info(4 * B);
    r.S = timed_paths(B, v_max, a_max, max_samples, info, r.q_traj, r.v_traj, [&](int S, double* traj, double* vel) {
      check(loikb_retime_paths(h_, q_path.data(), len, (int)B, T, 0, v_max.data(), a_max.data(), &p, S, traj, vel, r.seg.data(), r.duration.data(),
                               info.data(), 0));
    });
    split_info(info, 4, {&r.n_samples, &r.n_waypoints, &r.moved, &r.flags});
    return r;
  }
  // ---- blending (include/loik_amd_blend.h).  BlendPaths: RetimePaths through the corners -- every corner is replaced by a parabola of
  // half-length at most `reach` (halved up to max_tries - 1 times) when the advancement of MotionClearance certifies the curve at a
  // clearance >= margin, and is run through at a constant rate; a corner that is not certified stops.  max_samples as RetimePaths
  struct BlendResult {
    int S = 0;                                            // rows of q_traj / v_traj per path
    DVec q_traj, v_traj;                                  // [B][S][nq], [B][S][nv]
    std::vector<int> n_samples, n_waypoints, taken, flags;   // [B]; flags: LOIKB_BLEND_TRUNCATED / INVALID / SKIPPED
    DVec duration;                                        // [B]
    DVec corner;                                          // [B][T-2][5] = (l, r_in, r_out, rate, min_sampled)
    std::vector<int> corner_info;                         // [B][T-2][6] = (status LOIKB_BLEND_*, tries, evals, witness kind, a, b)
    DVec piece;                                           // [B][2T-3][4] = (t_start, duration, v0 or rate, v1 or rate)
  };
  BlendResult BlendPaths(const DVec& q_path, int T, const DVec& v_max, const DVec& a_max, double dt, double reach,
                         const std::vector<int>& n_waypoints = {}, int max_samples = -1, double margin = 0.0, double tol = 1e-3,
                         int max_evals = 256, int max_tries = 4) const
  {
    const std::size_t B = path_count(q_path, T, n_waypoints);
    const loikb_blend_params p{margin, tol, reach, dt, max_evals, max_tries, 0};
    const int* len = n_waypoints.empty() ? nullptr : n_waypoints.data();
    const std::size_t nc = T > 2 ? (std::size_t)T - 2 : 0, np = T > 1 ? 2 * (std::size_t)T - 3 : 0;
    BlendResult r;
    r.duration.resize(B);
    r.corner.resize(5 * B * nc);
    r.corner_info.resize(6 * B * nc);
    r.piece.resize(4 * B * np);
    std::vector<int> info(4 * B);
    r.S = timed_paths(B, v_max, a_max, max_samples, info, r.q_traj, r.v_traj, [&](int S, double* traj, double* vel) {
      check(loikb_blend_paths(h_, q_path.data(), len, (int)B, T, 0, v_max.data(), a_max.data(), &p, S, traj, vel, r.duration.data(), info.data(),
                              r.corner.data(), r.corner_info.data(), r.piece.data(), 0));
    });
    split_info(info, 4, {&r.n_samples, &r.n_waypoints, &r.taken, &r.flags});
    return r;
  }
  // ---- planning (include/loik_amd_plan.h).  PlanPaths: certified RRT-Connect from q_start [B][nq] to q_goal [B][nq]; two trees per query
  // grow towards samples drawn from the ranges s_lo, s_hi [nv] (a DoF is sampled iff both are finite) by edges of at most `step`, and every
  // edge is accepted only when the check of MotionClearance certifies it FREE.  T = the rows of a result path
  struct PlanResult {
    DVec q_path;                         // [B][T][nq]: NaN unless FOUND; the rows after n_waypoints repeat the last
    std::vector<int> n_waypoints, status, iterations;   // [B]; status: LOIKB_PLAN_*
    std::vector<int> nodes;              // [B][2]: the nodes of the start tree and of the goal tree
    std::vector<int> edges_checked, edges_free, evals;  // [B]
    DVec length;                         // [B], as PathLength; NaN unless FOUND
  };
  PlanResult PlanPaths(const DVec& q_start, const DVec& q_goal, const DVec& s_lo, const DVec& s_hi, int T, double step = 0.5, int max_iters = 256,
                       int max_nodes = 256, unsigned long long seed = 0, double margin = 0.0, double tol = 1e-3, int max_evals = 256) const
  {
    const std::size_t nq = (std::size_t)model_.nq, B = nq ? q_start.size() / nq : 0;
    if (q_start.size() != B * nq || q_goal.size() != q_start.size()) throw std::runtime_error("loik_amd: q_start and q_goal must hold the same whole number of rows of nq");
    if (s_lo.size() != (std::size_t)model_.nv || s_hi.size() != (std::size_t)model_.nv)
      throw std::runtime_error("loik_amd: s_lo and s_hi must hold model.nv values");
    const loikb_plan_params p{margin, tol, step, seed, max_evals, max_iters, max_nodes, 0};
    PlanResult r;
    r.q_path.resize(B * (std::size_t)(T > 0 ? T : 0) * nq);
    r.length.resize(B);
    std::vector<int> info(8 * B);
    check(loikb_plan_paths(h_, q_start.data(), q_goal.data(), (int)B, 0, s_lo.data(), s_hi.data(), &p, T, r.q_path.data(), info.data(), r.length.data(), 0));
    split_info<int>(info, 8, {&r.status, &r.n_waypoints, &r.iterations, nullptr, nullptr, &r.edges_checked, &r.edges_free, &r.evals});
    r.nodes.resize(2 * B);
    for (std::size_t b = 0; b < B; ++b) { r.nodes[2 * b] = info[8 * b + 3]; r.nodes[2 * b + 1] = info[8 * b + 4]; }
    return r;
  }
  // ---- collision avoidance (include/loik_amd_avoid.h): every later pose loop narrows the velocity box of each step so that the spheres
  // keep away from the world and from each other; clear: as if never set.  CollisionAvoidance(&p) returns whether it is set
  void SetCollisionAvoidance(double d_safe, double d_influence, double kappa = 0.5)
  {
    const loikb_avoid_params p{d_safe, d_influence, kappa, 0};
    check(loikb_avoid_set(h_, &p));
  }
  void ClearCollisionAvoidance() { check(loikb_avoid_set(h_, nullptr)); }
  bool CollisionAvoidance(loikb_avoid_params* p = nullptr) const { return loikb_avoid_get(h_, p) != 0; }
  struct AvoidResult {
    DVec min_seen;                        // [batch] the least clearance at the start of any step the instance ran
    std::vector<int> active_steps, flags; // [batch], [batch][nv] (bit 0: lower side narrowed, bit 1: upper side)
  };
  // of the last pose loop, which ran with collision avoidance set
  AvoidResult AvoidanceResult() const
  {
    AvoidResult r;
    r.min_seen.resize(batch_); r.active_steps.resize(batch_); r.flags.resize((std::size_t)batch_ * model_.nv);
    check(loikb_avoid_get_result(h_, LOIKB_AVOID_F_MIN_SEEN, r.min_seen.data(), 0));
    check(loikb_avoid_get_result(h_, LOIKB_AVOID_F_ACTIVE_STEPS, r.active_steps.data(), 0));
    check(loikb_avoid_get_result(h_, LOIKB_AVOID_F_FLAGS, r.flags.data(), 0));
    return r;
  }
  struct ClearanceGradientResult {
    ClearanceResult clearance;   // as Clearance()
    DVec grad;                   // [n][nv]: d(min)/dt = grad . z under Integrate
  };
  ClearanceGradientResult ClearanceGradient(const DVec* q = nullptr) const
  {
    const std::size_t n = q ? q->size() / (std::size_t)model_.nq : (std::size_t)batch_;
    if (q && q->size() != n * (std::size_t)model_.nq) throw std::runtime_error("loik_amd: q is not a whole number of configurations");
    DVec m(3 * n);
    ClearanceGradientResult r;
    r.clearance.witness.resize(3 * n);
    r.grad.resize(n * (std::size_t)model_.nv);
    check(loikb_clearance_gradient(h_, q ? q->data() : nullptr, (int)n, 0, m.data(), r.clearance.witness.data(), r.grad.data(), 0));
    r.clearance.min.resize(n); r.clearance.min_world.resize(n); r.clearance.min_self.resize(n);
    for (std::size_t i = 0; i < n; ++i) { r.clearance.min[i] = m[3 * i]; r.clearance.min_world[i] = m[3 * i + 1]; r.clearance.min_self[i] = m[3 * i + 2]; }
    return r;
  }
  struct AvoidanceBoxResult {
    DVec lo, hi;                 // [n][nv]
    DVec pairs;                  // [n][ns][2]: each sphere's nearest-world and nearest-self clearance
    std::vector<int> partner;    // [n][ns][2]: the world object (spheres first, then nws + box) / the other sphere, or -1
  };
  // the box a pose step with collision avoidance would hand its inner solve, for a shared [lb, ub] [nv]; q = nullptr: the resident q
  AvoidanceBoxResult AvoidanceBox(const DVec* q, double dt, const DVec& lb, const DVec& ub, double d_safe, double d_influence, double kappa = 0.5) const
  {
    const std::size_t n = q ? q->size() / (std::size_t)model_.nq : (std::size_t)batch_;
    if (q && q->size() != n * (std::size_t)model_.nq) throw std::runtime_error("loik_amd: q is not a whole number of configurations");
    if (lb.size() != (std::size_t)model_.nv || ub.size() != (std::size_t)model_.nv) throw std::runtime_error("loik_amd: lb and ub are [nv]");
    const loikb_avoid_params p{d_safe, d_influence, kappa, 0};
    AvoidanceBoxResult r;
    r.lo.resize(n * (std::size_t)model_.nv); r.hi.resize(n * (std::size_t)model_.nv);
    r.pairs.resize(2 * n * nspheres_); r.partner.resize(2 * n * nspheres_);
    check(loikb_avoid_box(h_, q ? q->data() : nullptr, (int)n, 0, dt, lb.data(), ub.data(), &p, r.lo.data(), r.hi.data(), r.pairs.data(), r.partner.data(), 0));
    return r;
  }
  // ---- multi-start pose IK (include/loik_amd_multistart.h): batch = G goals * K seeds, instance g * K + k is seed k of goal g
  // the ranges [nv] the seeds are drawn from (a DoF is sampled iff both ends are finite; both empty = the joint limits) and the
  // weights [nv] of the nearest-seed metric (empty = 1)
  void setSeedRanges(const DVec& s_lo = {}, const DVec& s_hi = {}, const DVec& weights = {})
  {
    if (s_lo.size() != s_hi.size() || (!weights.empty() && !s_lo.empty() && weights.size() != s_lo.size()))
      throw std::runtime_error("loik_amd: s_lo, s_hi and weights differ in size");
    check(loikb_multistart_set_ranges(h_, s_lo.empty() ? nullptr : s_lo.data(), s_hi.empty() ? nullptr : s_hi.data(),
                                      weights.empty() ? nullptr : weights.data(), (int)(s_lo.empty() ? weights.size() : s_lo.size())));
  }
  // writes the seeds of `round` into the resident q of all instances and nothing else.  q0: [G][nq], [nq] = one row for every
  // goal, nullptr = the resident q of each goal's instance g * K
  void SampleSeeds(int seeds_per_goal, unsigned long long seed = 0, int round = 0, const DVec* q0 = nullptr)
  {
    check(loikb_multistart_sample(h_, q0 ? q0->data() : nullptr, q0_flags(q0, seeds_per_goal), seed, seeds_per_goal, round));
  }
  struct MultiStartResult {
    std::vector<int> winner, goal_status, nreached;  // [G]; goal_status: LOIKB_MS_GOAL_* bits
    std::vector<int> round;                          // [batch]
    DVec q, err, cost;                               // [G][nq], [G][nc][6], [G]
    int rounds_run = 0;
    std::array<double, 6> timing{};                  // LOIKB_MS_F_TIMING
    // with setMultiStartClearance (include/loik_amd_collision.h), else empty: the winner's clearance and witness, the goal's clear seeds
    DVec clearance;                                  // [G]
    std::vector<int> witness, nclear;                // [G][3], [G]
  };
  // targets: one per goal and active constraint (G * nc, goal-major), or nc shared by the goals; q0 as SampleSeeds takes it
  MultiStartResult SolvePoseMultiStart(const std::vector<SE3>& targets, int seeds_per_goal, int rounds = 1, unsigned long long seed = 0,
                                       int pick = LOIKB_MS_PICK_NEAREST, const DVec* q0 = nullptr, double dt = 1.0, double gain = 1.0,
                                       double tol_pose = 1e-6, int max_steps = 100)
  {
    const std::size_t nc = (std::size_t)loikb_num_eq_c(h_);
    const bool k_ok = seeds_per_goal >= 1 && batch_ % seeds_per_goal == 0;   // (else the library says what is wrong with it)
    const std::size_t G = k_ok ? (std::size_t)(batch_ / seeds_per_goal) : 1;
    int flags = q0_flags(q0, seeds_per_goal);
    if (targets.size() == nc && G > 1) flags |= LOIKB_POSE_TARGET_SHARED;
    else if (targets.size() != G * nc)
      throw std::runtime_error("loik_amd: SolvePoseMultiStart needs one target per active constraint, shared or per goal");
    DVec t(targets.size() * 12);
    for (std::size_t i = 0; i < targets.size(); ++i) std::copy(targets[i].begin(), targets[i].end(), t.begin() + 12 * i);
    const loikb_pose_params p{dt, gain, tol_pose, max_steps, 0};
    const loikb_multistart_params m{seeds_per_goal, rounds, seed, pick, 0};
    check(loikb_solve_pose_multistart(h_, q0 ? q0->data() : nullptr, t.data(), flags, &p, &m));
    solved();
    MultiStartResult r;
    r.winner.resize(G); r.goal_status.resize(G); r.nreached.resize(G); r.round.resize(batch_);
    r.q.resize(G * model_.nq); r.err.resize(G * nc * 6); r.cost.resize(G);
    check(loikb_multistart_get(h_, LOIKB_MS_F_WINNER, r.winner.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_GOAL_STATUS, r.goal_status.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_NREACHED, r.nreached.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_ROUND, r.round.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_Q, r.q.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_ERR, r.err.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_COST, r.cost.data(), 0));
    check(loikb_multistart_get(h_, LOIKB_MS_F_TIMING, r.timing.data(), 0));
    r.rounds_run = (int)r.timing[0];
    if (MultiStartClearance()) {
      r.clearance.resize(G); r.witness.resize(3 * G); r.nclear.resize(G);
      check(loikb_clearance_get_multistart_result(h_, LOIKB_CLR_MS_F_CLEARANCE, r.clearance.data(), 0));
      check(loikb_clearance_get_multistart_result(h_, LOIKB_CLR_MS_F_WITNESS, r.witness.data(), 0));
      check(loikb_clearance_get_multistart_result(h_, LOIKB_CLR_MS_F_NCLEAR, r.nclear.data(), 0));
    }
    return r;
  }
  // ---- waypoint paths (include/loik_amd_path.h): SolvePose along T waypoints per instance, each instance at its own pace
  struct PathResult {
    std::vector<int> reached, cursor, steps, status, path_status;  // [batch]; status: LOIKB_POSE_ST_*, path_status: LOIKB_PATH_ST_* bits
    std::vector<int> wsteps;                                       // [batch][T]: steps spent on each waypoint
    DVec err;                                                      // [batch][nc][6]: against waypoint min(cursor, T - 1)
    DVec q_path;                                                   // [batch][T][nq], NaN rows from the cursor on; empty without record
    int n_waypoints = 0;
    std::array<double, 4> timing{};                                // LOIKB_PATH_F_TIMING
  };
  // waypoints: T * nc (waypoint-major) for the whole batch, or batch * T * nc instance-major; max_steps bounds the whole path,
  // max_steps_per_waypoint (0: no bound) one waypoint; q as SolvePose takes it
  PathResult SolvePosePath(const std::vector<SE3>& waypoints, int n_waypoints, double dt = 1.0, double gain = 1.0, double tol_pose = 1e-6,
                           int max_steps = 100, int max_steps_per_waypoint = 0, bool record = true, const DVec* q = nullptr)
  {
    const std::size_t nc = (std::size_t)loikb_num_eq_c(h_), T = (std::size_t)(n_waypoints > 0 ? n_waypoints : 1);
    int flags = 0;
    if (waypoints.size() == T * nc && batch_ > 1) flags |= LOIKB_POSE_TARGET_SHARED;
    else if (waypoints.size() != (std::size_t)batch_ * T * nc)
      throw std::runtime_error("loik_amd: SolvePosePath needs n_waypoints placements per active constraint, shared or per instance");
    if (q && q->size() != (std::size_t)batch_ * model_.nq) throw std::runtime_error("loik_amd: q must hold batch * model.nq values");
    DVec t(waypoints.size() * 12);
    for (std::size_t i = 0; i < waypoints.size(); ++i) std::copy(waypoints[i].begin(), waypoints[i].end(), t.begin() + 12 * i);
    const loikb_pose_params p{dt, gain, tol_pose, max_steps, 0};
    const loikb_path_params w{n_waypoints, max_steps_per_waypoint, record ? 1 : 0, 0};
    check(loikb_solve_pose_path(h_, q ? q->data() : nullptr, t.data(), flags, &p, &w));
    solved();
    PathResult r;
    r.n_waypoints = n_waypoints;
    r.steps.resize(batch_); r.status.resize(batch_); r.reached.resize(batch_); r.cursor.resize(batch_); r.path_status.resize(batch_);
    r.wsteps.resize((std::size_t)batch_ * T); r.err.resize((std::size_t)batch_ * nc * 6);
    check(loikb_pose_get(h_, LOIKB_POSE_F_STEPS, r.steps.data(), 0));
    check(loikb_pose_get(h_, LOIKB_POSE_F_STATUS, r.status.data(), 0));
    check(loikb_pose_get(h_, LOIKB_POSE_F_ERR, r.err.data(), 0));
    check(loikb_path_get(h_, LOIKB_PATH_F_CURSOR, r.cursor.data(), 0));
    check(loikb_path_get(h_, LOIKB_PATH_F_STATUS, r.path_status.data(), 0));
    check(loikb_path_get(h_, LOIKB_PATH_F_WSTEPS, r.wsteps.data(), 0));
    check(loikb_path_get(h_, LOIKB_PATH_F_TIMING, r.timing.data(), 0));
    if (record) {
      r.q_path.resize((std::size_t)batch_ * T * model_.nq);
      check(loikb_path_get(h_, LOIKB_PATH_F_Q, r.q_path.data(), 0));
    }
    for (int b = 0; b < batch_; ++b) r.reached[b] = (r.status[b] & LOIKB_POSE_ST_REACHED) ? 1 : 0;
    return r;
  }
  // ---- timed trajectories (include/loik_amd_track.h): closed-loop tracking of T + 1 samples per instance spaced dt apart, one inner
  // solve per step, every instance in step with the clock
  struct TrackResult {
    std::vector<int> steps, status, ontrack, worst_at;  // [batch]; status: LOIKB_POSE_ST_* bits (REACHED is never set)
    std::vector<int> inner;                             // [batch][T]: 1 = not converged, 2 = primal infeasible, 4 = a joint limit cut the box, 8 = an acceleration limit did
    DVec err;                                           // [batch][nc][6]: against X_T
    DVec errmax, worst;                                 // [batch][T+1], [batch]
    DVec q_traj, z_traj;                                // [batch][T+1][nq], [batch][T][nv], NaN rows after a stop; empty when not recorded
    int n_steps = 0;
    std::array<double, 4> timing{};                     // LOIKB_TRACK_F_TIMING
  };
  // samples: (T + 1) * nc (sample-major) for the whole batch, or batch * (T + 1) * nc instance-major; feedforward: LOIKB_TRACK_FF_*;
  // record: LOIKB_TRACK_REC_* bits; q as SolvePose takes it
  TrackResult TrackPose(const std::vector<SE3>& samples, int n_steps, double dt = 1.0, double gain = 1.0, double tol_track = 1e-4,
                        int feedforward = LOIKB_TRACK_FF_DIFFERENCE, int record = LOIKB_TRACK_REC_Q | LOIKB_TRACK_REC_Z, const DVec* q = nullptr)
  {
    const std::size_t nc = (std::size_t)loikb_num_eq_c(h_), T = (std::size_t)(n_steps > 0 ? n_steps : 1);
    int flags = 0;
    if (samples.size() == (T + 1) * nc && batch_ > 1) flags |= LOIKB_POSE_TARGET_SHARED;
    else if (samples.size() != (std::size_t)batch_ * (T + 1) * nc)
      throw std::runtime_error("loik_amd: TrackPose needs n_steps + 1 placements per active constraint, shared or per instance");
    if (q && q->size() != (std::size_t)batch_ * model_.nq) throw std::runtime_error("loik_amd: q must hold batch * model.nq values");
    DVec t(samples.size() * 12);
    for (std::size_t i = 0; i < samples.size(); ++i) std::copy(samples[i].begin(), samples[i].end(), t.begin() + 12 * i);
    const loikb_track_params p{dt, gain, tol_track, n_steps, feedforward, record, 0};
    check(loikb_track_pose(h_, q ? q->data() : nullptr, t.data(), flags, &p));
    solved();
    TrackResult r;
    r.n_steps = n_steps;
    r.steps.resize(batch_); r.status.resize(batch_); r.ontrack.resize(batch_); r.worst_at.resize(batch_); r.worst.resize(batch_);
    r.inner.resize((std::size_t)batch_ * T); r.errmax.resize((std::size_t)batch_ * (T + 1)); r.err.resize((std::size_t)batch_ * nc * 6);
    check(loikb_pose_get(h_, LOIKB_POSE_F_STEPS, r.steps.data(), 0));
    check(loikb_pose_get(h_, LOIKB_POSE_F_STATUS, r.status.data(), 0));
    check(loikb_pose_get(h_, LOIKB_POSE_F_ERR, r.err.data(), 0));
    check(loikb_track_get(h_, LOIKB_TRACK_F_ERRMAX, r.errmax.data(), 0));
    check(loikb_track_get(h_, LOIKB_TRACK_F_INNER, r.inner.data(), 0));
    check(loikb_track_get(h_, LOIKB_TRACK_F_ONTRACK, r.ontrack.data(), 0));
    check(loikb_track_get(h_, LOIKB_TRACK_F_WORST, r.worst.data(), 0));
    check(loikb_track_get(h_, LOIKB_TRACK_F_WORST_AT, r.worst_at.data(), 0));
    check(loikb_track_get(h_, LOIKB_TRACK_F_TIMING, r.timing.data(), 0));
    if (record & LOIKB_TRACK_REC_Q) {
      r.q_traj.resize((std::size_t)batch_ * (T + 1) * model_.nq);
      check(loikb_track_get(h_, LOIKB_TRACK_F_Q, r.q_traj.data(), 0));
    }
    if (record & LOIKB_TRACK_REC_Z) {
      r.z_traj.resize((std::size_t)batch_ * T * model_.nv);
      check(loikb_track_get(h_, LOIKB_TRACK_F_Z, r.z_traj.data(), 0));
    }
    return r;
  }
  // the resident configurations, [batch][nq]
  DVec q_resident() const
  {
    DVec q((std::size_t)batch_ * model_.nq);
    check(loikb_get(h_, LOIKB_F_Q, q.data(), 0));
    return q;
  }

  // ---- the logged lists of instance b (constructor argument logging = true; such a solver runs on the plain pass-by-pass
  //      implementation: "logging residuals, should be disabled for speed", loik-loid-optimized.hpp:408)
  LoikSolverInfo get_solver_info(int b = 0) const
  {
    LoikSolverInfo info;
    // (rows per instance as the library stored them: max_iter - 1 at the time of that solve, whatever set_max_iter did since)
    const std::size_t cap = static_cast<std::size_t>(std::max(loikb_solver_info_rows_cap(h_), 1));
    DVec buf(static_cast<std::size_t>(batch_) * cap);
    std::vector<int> rows(static_cast<std::size_t>(batch_));
    std::vector<double>* lists[] = {&info.primal_residual_task_list_, &info.primal_residual_slack_list_, &info.primal_residual_list_,
                                    &info.dual_residual_nu_list_, &info.dual_residual_v_list_, &info.dual_residual_list_,
                                    &info.mu_list_, &info.mu_eq_list_, &info.mu_ineq_list_};
    for (int l = 0; l < LOIKB_LOG_NLIST; ++l) {
      check(loikb_get_solver_info(h_, l, buf.data(), static_cast<int>(cap), rows.data()));
      lists[l]->assign(buf.begin() + b * cap, buf.begin() + b * cap + rows[b]);
    }
    const int n_iter = get_iter(b), n_tail = n_iter - rows[b];   // the tail solve extends iter_list_ only (hpp:286-290)
    for (int i = 1; i <= n_iter; ++i) info.iter_list_.push_back(i);
    for (int i = 1; i <= n_tail; ++i) info.tail_solve_iter_list_.push_back(i);
    return info;
  }

  // ---- which members of the data object every solve copies back (default: all six, as upstream's callers expect).
  // FETCH_NONE leaves the results on the device: read them with loikb_get(handle(), field, ptr, LOIKB_OUT_DEVICE) or call
  // fetch_now(mask) when needed -- a planner that only integrates on the device (Integrate) never needs the copy.
  enum : unsigned { FETCH_NONE = 0, FETCH_Z = 1, FETCH_NU = 2, FETCH_W = 4, FETCH_VIS = 8, FETCH_FIS = 16, FETCH_YIS = 32,
                    FETCH_ALL = 63 };
  void set_fetch(unsigned mask) { fetch_mask_ = mask; }
  unsigned get_fetch() const { return fetch_mask_; }
  void fetch_now(unsigned mask) { fetch(mask); }

  // task-solver-base.hpp:87-141 (instance index defaults to 0: the single-instance reading).  The per-instance scalars of
  // a solve are downloaded once, on the first getter call after it, and served from that copy: O(1) per call.
  int get_iter(int b = 0) const { return geti(LOIKB_F_ITER, b); }
  double get_primal_residual(int b = 0) const { return getd(LOIKB_F_PRIMAL_RESIDUAL, b); }
  double get_dual_residual(int b = 0) const { return getd(LOIKB_F_DUAL_RESIDUAL, b); }
  bool get_convergence_status(int b = 0) const { return geti(LOIKB_F_CONVERGED, b) != 0; }
  bool get_primal_infeasibility_status(int b = 0) const { return geti(LOIKB_F_PRIMAL_INFEASIBLE, b) != 0; }
  bool get_dual_infeasibility_status(int = 0) const { return false; }  // never set by the optimized solver upstream
  double get_mu(int b = 0) const { return getd(LOIKB_F_MU, b); }
  double get_rho() const { return rho_; }
  // set_tol_primal / set_tol_dual (task-solver-base.hpp:118-127) write tol_primal_ / tol_dual_, which CheckConvergence
  // recomputes at every iteration (hxx:544-552): as upstream, the value set is what the getter returns until the next solve
  double get_tol_primal(int b = 0) const { return tol_primal_set_ ? tol_primal_ : getd(LOIKB_F_TOL_PRIMAL, b); }
  double get_tol_dual(int b = 0) const { return tol_dual_set_ ? tol_dual_ : getd(LOIKB_F_TOL_DUAL, b); }
  void set_tol_primal(const double t) { tol_primal_ = t; tol_primal_set_ = true; }
  void set_tol_dual(const double t) { tol_dual_ = t; tol_dual_set_ = true; }
  double get_tol_primal_inf() const { return tol_primal_inf_; }
  double get_tol_dual_inf() const { return tol_dual_inf_; }
  void set_max_iter(const int max_iter) { check(loikb_set_max_iter(h_, max_iter)); max_iter_ = max_iter; }
  void set_rho(const double rho) { rho_ = rho; check(loikb_set_rho(h_, rho)); }
  void set_mu(const double mu) { check(loikb_set_mu(h_, mu)); }
  void set_tol_primal_inf(const double t) { tol_primal_inf_ = t; check(loikb_set_tol_primal_inf(h_, t)); }
  // dual infeasibility is never evaluated on this path: the tolerance is stored, as upstream stores it
  void set_tol_dual_inf(const double t) { tol_dual_inf_ = t; }
  // loik-loid-optimized.hpp:700-755
  // get_primal_residual_vec() / get_dual_residual_vec(), loik-loid-optimized.hpp:698-699: [6 nb + nv] of instance b
  DVec get_primal_residual_vec(int b = 0) const { return getvec(LOIKB_F_PRIMAL_RESIDUAL_VEC, b); }
  DVec get_dual_residual_vec(int b = 0) const { return getvec(LOIKB_F_DUAL_RESIDUAL_VEC, b); }
  double get_dual_residual_v(int b = 0) const { return getd(LOIKB_F_DUAL_RESIDUAL_V, b); }
  double get_dual_residual_nu(int b = 0) const { return getd(LOIKB_F_DUAL_RESIDUAL_NU, b); }
  double get_tol_tail_solve() const { return tol_tail_solve_; }
  void set_tol_tail_solve(const double tol) { tol_tail_solve_ = tol; check(loikb_set_tol_tail_solve(h_, tol)); }
  double get_delta_x_qp_inf_norm(int b = 0) const { return getd(LOIKB_F_DELTA_X_QP_INF_NORM, b); }
  double get_delta_z_qp_inf_norm(int b = 0) const { return getd(LOIKB_F_DELTA_Z_QP_INF_NORM, b); }
  double get_delta_y_qp_inf_norm(int b = 0) const { return getd(LOIKB_F_DELTA_Y_QP_INF_NORM, b); }
  double get_A_qp_T_delta_y_qp_inf_norm(int b = 0) const { return getd(LOIKB_F_A_QP_T_DELTA_Y_QP_INF_NORM, b); }
  double get_ub_qp_T_delta_y_qp_plus(int b = 0) const { return getd(LOIKB_F_UB_QP_T_DELTA_Y_QP_PLUS, b); }
  double get_lb_qp_T_delta_y_qp_minus(int b = 0) const { return getd(LOIKB_F_LB_QP_T_DELTA_Y_QP_MINUS, b); }
  bool get_primal_infeasibility_cond_1(int b = 0) const { return getd(LOIKB_F_PRIMAL_INFEASIBILITY_COND_1, b) != 0.0; }
  bool get_primal_infeasibility_cond_2(int b = 0) const { return getd(LOIKB_F_PRIMAL_INFEASIBILITY_COND_2, b) != 0.0; }

  loikb_stats stats() const
  {
    loikb_stats s{};
    loikb_get_stats(h_, &s);
    return s;
  }
  loikb_solver* handle() const { return h_; }

private:
  struct Args {
    std::vector<int> ids;
    DVec A, b;
    int flags = 0, nbound = 0;
    Args(const FirstOrderLoikOptimized& s, const DVec& q, const std::vector<Index>& cids, const std::vector<Mat6x6>& Ais,
         const std::vector<Vec6>& bis, const DVec& lb, const DVec& ub)
    {
      // same consistency checks, same messages as ik-id-description-optimized.hpp:132-151, :328-335
      if (lb.size() != ub.size())
        throw std::runtime_error("[IkProblemFormulation::UpdateIneqConstraints]: lower bound and upper bound have different dimensions!!!");
      const std::size_t nc = cids.size(), B = static_cast<std::size_t>(s.batch_);
      if (!(Ais.size() == nc || Ais.size() == nc * B) || !(bis.size() == nc || bis.size() == nc * B))
        throw std::runtime_error("[IkProblemFormulation::UpdateEqConstraints]: task_constraint_ids, Ais, and bis have different size !!!");
      for (Index c : cids) ids.push_back(static_cast<int>(c));
      A.resize(Ais.size() * 36);
      for (std::size_t i = 0; i < Ais.size(); ++i)
        for (int k = 0; k < 36; ++k) A[36 * i + k] = Ais[i][k];
      b.resize(bis.size() * 6);
      for (std::size_t i = 0; i < bis.size(); ++i)
        for (int k = 0; k < 6; ++k) b[6 * i + k] = bis[i][k];
      if (Ais.size() == nc) flags |= LOIKB_A_SHARED;
      if (bis.size() == nc && B > 1) flags |= LOIKB_B_SHARED;
      const std::size_t nv = static_cast<std::size_t>(s.model_.nv);
      if (lb.size() == nv * B && B > 1) nbound = (int)nv;
      else { nbound = (int)lb.size(); flags |= LOIKB_BOUNDS_SHARED; }
      const std::size_t nq = static_cast<std::size_t>(s.model_.nq);
      if (q.size() != nq && q.size() != nq * B)   // (the C-ABI takes bare pointers: sizes are checked here)
        throw std::runtime_error("loik_amd: q must hold model.nq values (one configuration for the batch) or batch * model.nq");
      if (B > 1 && q.size() == nq) flags |= LOIKB_Q_SHARED;
    }
  };

  void check_q(const DVec& q) const
  {
    const std::size_t nq = static_cast<std::size_t>(model_.nq);
    if (q.size() != nq && q.size() != nq * static_cast<std::size_t>(batch_))
      throw std::runtime_error("loik_amd: q must hold model.nq values (one configuration for the batch) or batch * model.nq");
  }
  static DVec flat(const std::vector<Vec6>& bis)
  {
    DVec b(bis.size() * 6);
    for (std::size_t i = 0; i < bis.size(); ++i)
      for (int k = 0; k < 6; ++k) b[6 * i + k] = bis[i][k];
    return b;
  }
  void check_bis(const std::vector<Vec6>& bis) const
  {
    if (bis.size() != 1 && bis.size() != static_cast<std::size_t>(batch_))
      throw std::runtime_error("loik_amd: bis must hold one target (for the whole batch) or one per instance");
  }
  int b_flag(const std::vector<Vec6>& bis) const { check_bis(bis); return (bis.size() == 1 && batch_ > 1) ? LOIKB_B_SHARED : 0; }
  // yis / Aty of the data object follow nc_eq_ (upstream never resizes them: its AddEqConstraint is deactivated)
  void resize_constraints()
  {
    nc_ = loikb_num_eq_c(h_);
    ik_id_data_.num_eq_c = nc_;
    ik_id_data_.yis.assign(static_cast<std::size_t>(batch_) * nc_ * 6, 0.0);
    ik_id_data_.Aty.buf_.assign(static_cast<std::size_t>(batch_) * nc_ * 6, 0.0);
    ++generation_;
  }

  void check(int rc) const
  {
    if (rc == LOIKB_OK) return;
    const char* msg = (rc <= LOIKB_ERR_ARG || rc == LOIKB_ERR_MODEL) ? loikb_last_error() : loikb_status_string(rc);
    throw std::runtime_error(msg && *msg ? msg : loikb_status_string(rc));
  }
  // (include/loik_amd_depth.h) the parameters of a call from its options; *nf: the filter configurations
  loikb_depth_params depth_params_(const DepthOptions& opt, double voxel, int* nf) const
  {
    const std::size_t nq = (std::size_t)model_.nq, rows = opt.filter_q.size() / nq;
    if (opt.filter_q.size() != rows * nq) throw std::runtime_error("loik_amd: filter_q is not a whole number of configurations");
    *nf = opt.filter_q.empty() ? opt.filter_resident : (int)rows;
    const double cover = 0.5 * std::sqrt(3.0) * voxel;
    return loikb_depth_params{opt.fuse ? LOIKB_DEPTH_FUSE : LOIKB_DEPTH_REPLACE, opt.carve ? 1 : 0, opt.carve ? (opt.band < 0.0 ? cover : opt.band) : 0.0,
                              opt.filter_pad < 0.0 ? cover : opt.filter_pad, 0};
  }
  DepthStats integrate_depth_(const void* depth, std::size_t count, int type, const DepthCamera& cam, const std::array<int, 3>& dims,
                              const std::array<double, 3>& origin, double voxel, const DepthOptions& opt)
  {
    if (cam.width <= 0 || cam.height <= 0 || count != (std::size_t)cam.width * (std::size_t)cam.height)
      throw std::runtime_error("loik_amd: need width * height > 0 depth pixels");
    loikb_depth_camera c;
    c.width = cam.width; c.height = cam.height;
    c.fx = cam.fx; c.fy = cam.fy; c.cx = cam.cx; c.cy = cam.cy;
    for (int k = 0; k < 12; ++k) c.T_world_cam[k] = cam.T_world_cam[(std::size_t)k];
    c.depth_scale = cam.depth_scale; c.z_min = cam.z_min; c.z_max = cam.z_max;
    int nf = 0;
    const loikb_depth_params prm = depth_params_(opt, voxel, &nf);
    long long st[4] = {0, 0, 0, 0};
    check(loikb_collision_grid_integrate_depth(h_, depth, type, &c, dims.data(), origin.data(), voxel, &prm, opt.filter_q.empty() ? nullptr : opt.filter_q.data(), nf, 0, st));
    return DepthStats{st[0], st[1], st[2], st[3]};
  }
  void pass(int id)
  {
    check(loikb_pass(h_, id));
    solved();
  }
  void solved()
  {
    ++generation_;  // lazy members and cached scalars of the previous solve are stale now
    tol_primal_set_ = tol_dual_set_ = false;
    fetch(fetch_mask_);
  }
  void fetch(unsigned mask)
  {
    // (one call for all of them -- loikb_get_results: one gather launch and one synchronisation for a small batch; the FETCH_* bits are LOIKB_RES_*)
    static_assert(FETCH_Z == LOIKB_RES_Z && FETCH_NU == LOIKB_RES_NU && FETCH_W == LOIKB_RES_W && FETCH_VIS == LOIKB_RES_VIS &&
                  FETCH_FIS == LOIKB_RES_FIS && FETCH_YIS == LOIKB_RES_YIS, "fetch mask out of step with loikb_get_results");
    if (nc_ <= 0) mask &= ~static_cast<unsigned>(FETCH_YIS);
    mask &= FETCH_ALL;
    // A small batch (the fused gather of loikb_get_results will serve it): the scalars behind get_iter(), get_convergence_status(), the
    // residuals ... ride along -- a scalar getter's own device call costs 0.025 ms, one problem's callers make two or three after every solve.
    // A large batch keeps them lazy (one download per field that is actually asked for).
    const std::size_t per = 3 * static_cast<std::size_t>(model_.nv) + 12 * static_cast<std::size_t>(model_.njoints - 1) +
                            6 * static_cast<std::size_t>(nc_ > 0 ? nc_ : 0) + LOIKB_RES_NSCALARS;
    const bool with_scalars = mask != 0 && sizeof(double) * per * static_cast<std::size_t>(batch_) <= LOIKB_RESULTS_FUSED_BYTES_DEFAULT;
    if (with_scalars) scal_.resize(static_cast<std::size_t>(batch_) * LOIKB_RES_NSCALARS);
    if (mask)
      check(loikb_get_results(h_, mask | (with_scalars ? LOIKB_RES_SCALARS : 0u), ik_id_data_.z.data(), ik_id_data_.nu.data(), ik_id_data_.w.data(),
                              ik_id_data_.vis.data(), ik_id_data_.fis.data(), ik_id_data_.yis.data(), with_scalars ? scal_.data() : nullptr));
    if (with_scalars) {
      const std::size_t B = static_cast<std::size_t>(batch_);
      for (int k = 0; k < LOIKB_RES_SCALAR_ITER; ++k) {   // the 30 scalar fields, LOIKB_F_PRIMAL_RESIDUAL + k
        Cached<DVec>& c = dcache_[LOIKB_F_PRIMAL_RESIDUAL + k];
        c.data.resize(B);
        for (std::size_t b = 0; b < B; ++b) c.data[b] = scal_[b * LOIKB_RES_NSCALARS + static_cast<std::size_t>(k)];
        c.gen = generation_;
      }
      auto fill_int = [&](int field, int col, int mask_bits) {
        Cached<std::vector<int>>& c = icache_[field];
        c.data.resize(B);
        for (std::size_t b = 0; b < B; ++b) {
          const int v = static_cast<int>(scal_[b * LOIKB_RES_NSCALARS + static_cast<std::size_t>(col)]);
          c.data[b] = mask_bits ? ((v & mask_bits) ? 1 : 0) : v;
        }
        c.gen = generation_;
      };
      fill_int(LOIKB_F_ITER, LOIKB_RES_SCALAR_ITER, 0);
      fill_int(LOIKB_F_STATUS, LOIKB_RES_SCALAR_STATUS, 0);
      fill_int(LOIKB_F_CONVERGED, LOIKB_RES_SCALAR_STATUS, 1);
      fill_int(LOIKB_F_PRIMAL_INFEASIBLE, LOIKB_RES_SCALAR_STATUS, 2);
      fill_int(LOIKB_F_MU_UPDATES, LOIKB_RES_SCALAR_MU_UPDATES, 0);
    }
  }
  // one download per field and solve, then O(1) per getter call
  template <typename V>
  struct Cached { V data; unsigned long long gen = ~0ull; };
  int geti(int field, int b) const
  {
    Cached<std::vector<int>>& c = icache_[field];
    if (c.gen != generation_) {
      c.data.resize(static_cast<std::size_t>(batch_));
      check(loikb_get(h_, field, c.data.data(), 0));
      c.gen = generation_;
    }
    return c.data[static_cast<std::size_t>(b)];
  }
  double getd(int field, int b) const
  {
    Cached<DVec>& c = dcache_[field];
    if (c.gen != generation_) {
      c.data.resize(static_cast<std::size_t>(batch_));
      check(loikb_get(h_, field, c.data.data(), 0));
      c.gen = generation_;
    }
    return c.data[static_cast<std::size_t>(b)];
  }
  DVec getvec(int field, int b) const
  {
    const std::size_t n = 6 * static_cast<std::size_t>(model_.njoints - 1) + static_cast<std::size_t>(model_.nv);
    Cached<DVec>& c = dcache_[field];
    if (c.gen != generation_) {
      c.data.resize(static_cast<std::size_t>(batch_) * n);
      check(loikb_get(h_, field, c.data.data(), 0));
      c.gen = generation_;
    }
    return DVec(c.data.begin() + b * n, c.data.begin() + (b + 1) * n);
  }
  friend class LazyField;
  void lazy_fetch(int field, double* dst) const { check(loikb_get(h_, field, dst, 0)); }

  Model model_;             // by value, as upstream (loik-loid-optimized.hpp:762)
  IkIdData& ik_id_data_;    // caller-owned, must outlive the solver (loik-loid-optimized.hpp:763)
  // q0 of the multi-start entry points: [nq] = one shared row, [G][nq] = one per goal (G = 1: per goal)
  int q0_flags(const DVec* q0, int seeds_per_goal) const
  {
    if (!q0) return 0;
    const bool k_ok = seeds_per_goal >= 1 && batch_ % seeds_per_goal == 0;
    const std::size_t G = k_ok ? (std::size_t)(batch_ / seeds_per_goal) : 1;
    if (q0->size() == G * (std::size_t)model_.nq) return 0;
    if (q0->size() == (std::size_t)model_.nq) return LOIKB_Q_SHARED;
    throw std::runtime_error("loik_amd: q0 must hold model.nq values (shared by the goals) or goals * model.nq");
  }
  // B of q_path [B][T][nq] with n_waypoints [B] or empty
  std::size_t path_count(const DVec& q_path, int T, const std::vector<int>& n_waypoints) const
  {
    const std::size_t per = (std::size_t)(T > 0 ? T : 1) * (std::size_t)model_.nq, B = q_path.size() / per;
    if (q_path.size() != B * per) throw std::runtime_error("loik_amd: q_path is not a whole number of paths of T samples");
    if (!n_waypoints.empty() && n_waypoints.size() != B) throw std::runtime_error("loik_amd: n_waypoints is not one count per path");
    return B;
  }
  // column k of info [B][stride] into *cols[k], a nullptr skipping its column
  template <class T> static void split_info(const std::vector<T>& info, std::size_t stride, std::initializer_list<std::vector<T>*> cols)
  {
    const std::size_t B = info.size() / stride;
    std::size_t k = 0;
    for (std::vector<T>* c : cols) {
      if (c) c->resize(B);
      for (std::size_t b = 0; c && b < B; ++b) (*c)[b] = info[stride * b + k];
      ++k;
    }
  }
  // what RetimePaths and BlendPaths share: v_max and a_max checked, S = max_samples or, when that is < 0, the largest n_samples of a
  // timing-only call, traj and vel sized to S rows, then the real call.  call(S, traj, vel) is the C call, which fills info [B][4]
  template <class Call> int timed_paths(std::size_t B, const DVec& v_max, const DVec& a_max, int max_samples, const std::vector<int>& info, DVec& traj,
                                        DVec& vel, Call&& call) const
  {
    if (v_max.size() != (std::size_t)model_.nv || a_max.size() != (std::size_t)model_.nv)
      throw std::runtime_error("loik_amd: v_max and a_max must hold model.nv values");
    if (max_samples < 0) {
      call(0, nullptr, nullptr);
      max_samples = 1;
      for (std::size_t b = 0; b < B; ++b) max_samples = std::max(max_samples, info[4 * b]);
    }
    traj.resize(B * (std::size_t)max_samples * (std::size_t)model_.nq);
    vel.resize(B * (std::size_t)max_samples * (std::size_t)model_.nv);
    call(max_samples, max_samples > 0 ? traj.data() : nullptr, max_samples > 0 ? vel.data() : nullptr);
    return max_samples;
  }
  // out_val [n][3], out_info [n][5] of loik_amd_motion.h by field
  static MotionResult motion_result(const DVec& val, const std::vector<int>& info)
  {
    const std::size_t n = val.size() / 3;
    MotionResult r;
    r.status.resize(n); r.evals.resize(n); r.s_free.resize(n); r.min_sampled.resize(n); r.s_at_min.resize(n); r.witness.resize(3 * n);
    for (std::size_t i = 0; i < n; ++i) {
      r.s_free[i] = val[3 * i]; r.min_sampled[i] = val[3 * i + 1]; r.s_at_min[i] = val[3 * i + 2];
      r.status[i] = info[5 * i]; r.evals[i] = info[5 * i + 1];
      for (int k = 0; k < 3; ++k) r.witness[3 * i + k] = info[5 * i + 2 + k];
    }
    return r;
  }
  loikb_solver* h_ = nullptr;
  int batch_, nc_;
  std::size_t nspheres_ = 0;   // of the last setCollisionSpheres: AvoidanceBox sizes its per-sphere results by it
  int max_iter_ = 0;
  double rho_ = 0.0, tol_tail_solve_ = 0.0, tol_primal_inf_ = 0.0, tol_dual_inf_ = 0.0;
  double tol_primal_ = 0.0, tol_dual_ = 0.0;
  bool tol_primal_set_ = false, tol_dual_set_ = false;
  unsigned fetch_mask_ = FETCH_ALL;
  DVec scal_;   // [batch][LOIKB_RES_NSCALARS]: the scalar block of the last fused fetch
  unsigned long long generation_ = 1;
  mutable std::map<int, Cached<std::vector<int>>> icache_;
  mutable std::map<int, Cached<DVec>> dcache_;
};

inline const DVec& LazyField::get() const
{
  if (owner_ && generation_ && seen_ != *generation_) {
    owner_->lazy_fetch(field_, buf_.data());
    seen_ = *generation_;
  }
  return buf_;
}

}  // namespace loik_amd
