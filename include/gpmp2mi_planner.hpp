// gpmp2mi_planner.hpp -- header-only C++ host facade over the C ABI (include/gpmp2mi.h) that keeps the
// call shapes of gpmp2/planner so existing C++ callers can switch with a namespace change:
//
//   gpmp2::Arm, gpmp2::BodySphere, gpmp2::ArmModel      gpmp2/kinematics/Arm.h:48-59, RobotModel.h:20-90
//   gpmp2::SignedDistanceField, gpmp2::PlanarSDF        gpmp2/obstacle/SignedDistanceField.h:57-81, PlanarSDF.h:44-46
//   gpmp2::TrajOptimizerSetting                         gpmp2/planner/TrajOptimizerSetting.h:17-100
//   gpmp2::BatchTrajOptimize3DArm / 2DArm               gpmp2/planner/BatchTrajOptimizer.h:43-56
//   gpmp2::CollisionCost3DArm / 2DArm                   gpmp2/planner/BatchTrajOptimizer.h:135-147
//   gpmp2::Pose2MobileArm / Pose2MobileArmModel, BatchTrajOptimizePose2MobileArm(2D)   gpmp2/planner/BatchTrajOptimizer.h:57-73
//   gpmp2::Obstacle(Planar)SDFFactorArm / ...Pose2MobileArm, GoalFactorArm, GaussianPriorWorkspacePoseArm, SelfCollisionArm
//   gpmp2::interpolateArmTraj / interpolatePose2MobileArmTraj  gpmp2/planner/TrajUtils.cpp:96-236
//   gpmp2::ISAM2TrajOptimizer2DArm / 3DArm              gpmp2/planner/ISAM2TrajOptimizer.h:143-156
//   gpmp2::initArmTrajStraightLine                      gpmp2/planner/TrajUtils.cpp:25-50
//
// The reference passes gtsam::Values / gtsam::Vector / gtsam::Pose3.  GTSAM, Boost and Eigen are not part of
// this repository, so the facade uses plain std::vector containers (`Trajectory`, state i = [x_i; v_i]) and,
// where <gtsam/nonlinear/Values.h> is on the include path, also provides converters to and from
// gtsam::Values with the reference's key convention Symbol('x', i) / Symbol('v', i).
// Errors: the C ABI's status codes are rethrown as std::runtime_error, matching the reference's use of
// exceptions.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gpmp2mi.h"

#if defined(__has_include)
#if __has_include(<gtsam/nonlinear/Values.h>) && __has_include(<gtsam/inference/Symbol.h>)
#include <gtsam/inference/Symbol.h>
#include <gtsam/nonlinear/Values.h>
#define GPMP2MI_HAVE_GTSAM 1
#endif
#endif

namespace gpmp2mi {

using Vector = std::vector<double>;

inline void check(int rc, const char* what) {
  if (rc != GPMP2MI_OK)
    throw std::runtime_error(std::string("[gpmp2mi] ") + what + ": " + gpmp2mi_last_error() + " (code " +
                             std::to_string(rc) + ")");
}

/// 4x4 homogeneous transform, row-major (stand-in for gtsam::Pose3)
struct Pose3 {
  std::array<double, 16> m{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  static Pose3 Translation(double x, double y, double z) {
    Pose3 p;
    p.m[3] = x;
    p.m[7] = y;
    p.m[11] = z;
    return p;
  }
};

/// body sphere: attached link id, radius, centre in the link frame
struct BodySphere {
  std::size_t link_id;
  double radius;
  std::array<double, 3> center;
  BodySphere(std::size_t id, double r, const std::array<double, 3>& c) : link_id(id), radius(r), center(c) {}
};
using BodySphereVector = std::vector<BodySphere>;

/// DH arm, same constructor argument order as gpmp2::Arm
class Arm {
 public:
  Arm(std::size_t dof, const Vector& a, const Vector& alpha, const Vector& d, const Pose3& base_pose = Pose3(),
      const Vector& theta_bias = Vector())
      : dof_(dof), a_(a), alpha_(alpha), d_(d), base_(base_pose),
        bias_(theta_bias.empty() ? Vector(dof, 0.0) : theta_bias) {
    if (a.size() != dof || alpha.size() != dof || d.size() != dof || bias_.size() != dof)
      throw std::runtime_error("[Arm] DH parameter vector dim does not fit dof");
  }
  std::size_t dof() const { return dof_; }
  std::size_t nr_links() const { return dof_; }
  const Vector& a() const { return a_; }
  const Vector& alpha() const { return alpha_; }
  const Vector& d() const { return d_; }
  const Vector& theta_bias() const { return bias_; }
  const Pose3& base_pose() const { return base_; }

 private:
  std::size_t dof_;
  Vector a_, alpha_, d_;
  Pose3 base_;
  Vector bias_;
};

/// RobotModel<Arm>: owns the device-side robot handle
class ArmModel {
 public:
  ArmModel(const Arm& arm, const BodySphereVector& spheres) : arm_(arm), spheres_(spheres) {
    gpmp2mi_robot_desc d{};
    d.kind = GPMP2MI_ROBOT_ARM;
    d.dof = d.arm_dof = static_cast<int>(arm.dof());
    d.a = arm_.a().data();
    d.alpha = arm_.alpha().data();
    d.d = arm_.d().data();
    d.theta_bias = arm_.theta_bias().data();
    for (int i = 0; i < 16; i++) d.base_pose[i] = arm_.base_pose().m[i];
    std::vector<int> link;
    Vector radius, center;
    for (const auto& s : spheres_) {
      link.push_back(static_cast<int>(s.link_id));
      radius.push_back(s.radius);
      center.insert(center.end(), s.center.begin(), s.center.end());
    }
    d.nr_spheres = static_cast<int>(spheres_.size());
    d.sphere_link = link.data();
    d.sphere_radius = radius.data();
    d.sphere_center = center.data();
    check(gpmp2mi_robot_create(&d, &h_), "gpmp2mi_robot_create");
  }
  ArmModel(const ArmModel&) = delete;
  ArmModel& operator=(const ArmModel&) = delete;
  ~ArmModel() { gpmp2mi_robot_destroy(h_); }
  std::size_t dof() const { return arm_.dof(); }
  std::size_t nr_body_spheres() const { return spheres_.size(); }
  double sphere_radius(std::size_t i) const { return spheres_[i].radius; }
  const Arm& fk_model() const { return arm_; }
  const gpmp2mi_robot* handle() const { return h_; }

  /// RobotModel::sphereCentersMat -> [S][3]
  Vector sphereCenters(const Vector& conf) const {
    Vector out(3 * spheres_.size());
    check(gpmp2mi_sphere_centers(h_, 1, conf.data(), out.data(), nullptr), "gpmp2mi_sphere_centers");
    return out;
  }

 private:
  Arm arm_;
  BodySphereVector spheres_;
  gpmp2mi_robot* h_ = nullptr;
};

/// gpmp2::Pose2MobileArm  gpmp2/kinematics/Pose2MobileArm.h:22-70 (state [x, y, theta, q...])
class Pose2MobileArm {
 public:
  explicit Pose2MobileArm(const Arm& arm, const Pose3& base_T_arm = Pose3()) : arm_(arm), base_T_arm_(base_T_arm) {}
  std::size_t dof() const { return arm_.dof() + 3; }
  std::size_t nr_links() const { return arm_.dof() + 1; }
  const Arm& arm() const { return arm_; }
  const Pose3& base_T_arm() const { return base_T_arm_; }

 private:
  Arm arm_;
  Pose3 base_T_arm_;
};

/// RobotModel<Pose2MobileArm>: owns the device-side robot handle; sphere link 0 = vehicle base
class Pose2MobileArmModel {
 public:
  Pose2MobileArmModel(const Pose2MobileArm& marm, const BodySphereVector& spheres) : marm_(marm), spheres_(spheres) {
    gpmp2mi_robot_desc d{};
    d.kind = GPMP2MI_ROBOT_POSE2_MOBILE_ARM;
    d.dof = static_cast<int>(marm.dof());
    d.arm_dof = static_cast<int>(marm.arm().dof());
    d.a = marm_.arm().a().data();
    d.alpha = marm_.arm().alpha().data();
    d.d = marm_.arm().d().data();
    d.theta_bias = marm_.arm().theta_bias().data();
    for (int i = 0; i < 16; i++) {
      d.base_pose[i] = marm_.base_T_arm().m[i];
      d.base_pose2[i] = d.base_pose3[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    std::vector<int> link;
    Vector radius, center;
    for (const auto& sp : spheres_) {
      link.push_back(static_cast<int>(sp.link_id));
      radius.push_back(sp.radius);
      center.insert(center.end(), sp.center.begin(), sp.center.end());
    }
    d.nr_spheres = static_cast<int>(spheres_.size());
    d.sphere_link = link.data();
    d.sphere_radius = radius.data();
    d.sphere_center = center.data();
    check(gpmp2mi_robot_create(&d, &h_), "gpmp2mi_robot_create");
  }
  Pose2MobileArmModel(const Pose2MobileArmModel&) = delete;
  Pose2MobileArmModel& operator=(const Pose2MobileArmModel&) = delete;
  ~Pose2MobileArmModel() { gpmp2mi_robot_destroy(h_); }
  std::size_t dof() const { return marm_.dof(); }
  std::size_t nr_body_spheres() const { return spheres_.size(); }
  const Pose2MobileArm& fk_model() const { return marm_; }
  const gpmp2mi_robot* handle() const { return h_; }

 private:
  Pose2MobileArm marm_;
  BodySphereVector spheres_;
  gpmp2mi_robot* h_ = nullptr;
};

/// counts of a point cloud update (include/gpmp2mi.h "live map"): the four classes sum to the number of points
struct MapUpdateStats {
  int kept = 0, non_finite = 0, self = 0, outside = 0;
};

namespace internal {
/// gpmp2mi_sdf_update_from_points for the two field classes: points row-major [M][dim]
inline MapUpdateStats UpdateFieldFromPoints(gpmp2mi_sdf* h, std::size_t dim, const Vector& points, bool use_base,
                                            const gpmp2mi_robot* robot, const Vector* conf, double margin) {
  if (points.size() % dim != 0) throw std::runtime_error("[updateFromPoints] points are not [M][dim]");
  if (robot && (!conf || conf->size() != static_cast<std::size_t>(gpmp2mi_robot_dof(robot))))
    throw std::runtime_error("[updateFromPoints] conf does not fit the robot's dof");
  int st[4] = {0, 0, 0, 0};
  check(gpmp2mi_sdf_update_from_points(h, static_cast<int>(points.size() / dim), points.data(), use_base ? 1 : 0, robot,
                                       robot ? conf->data() : nullptr, margin, st),
        "gpmp2mi_sdf_update_from_points");
  MapUpdateStats s;
  s.kept = st[0];
  s.non_finite = st[1];
  s.self = st[2];
  s.outside = st[3];
  return s;
}
}  // namespace internal

/// counts of an integrate call (include/gpmp2mi.h "sensor map"): the five classes sum to the number of rays; `occupied`
/// is the number of cells whose evidence reaches occupied_at afterwards
struct EvidenceStats {
  int hit = 0, invalid = 0, max_range = 0, self = 0, outside = 0, occupied = 0;
};
/// gpmp2mi_evidence_opts with its defaults: hit 2, miss 1, lo -4, hi 8, occupied_at 1, use_base 0, refresh 1
struct EvidenceOptions : gpmp2mi_evidence_opts {
  EvidenceOptions() { gpmp2mi_evidence_opts_default(this); }
};
/// camera -> world pose, intrinsics and depth range of a depth image
using DepthCamera = gpmp2mi_depth_camera;

namespace internal {
inline EvidenceStats EvidenceStatsOf(const int (&st)[6]) {
  EvidenceStats s;
  s.hit = st[0];
  s.invalid = st[1];
  s.max_range = st[2];
  s.self = st[3];
  s.outside = st[4];
  s.occupied = st[5];
  return s;
}
/// gpmp2mi_sdf_integrate_points for the two field classes: points row-major [M][dim], sensor_origin [dim]
inline EvidenceStats IntegratePoints(gpmp2mi_sdf* h, std::size_t dim, const Vector& points, const Vector& sensor_origin,
                                     const gpmp2mi_evidence_opts& opts, const gpmp2mi_robot* robot, const Vector* conf,
                                     double margin) {
  if (points.size() % dim != 0) throw std::runtime_error("[integratePoints] points are not [M][dim]");
  if (sensor_origin.size() != dim) throw std::runtime_error("[integratePoints] sensor_origin is not [dim]");
  if (robot && (!conf || conf->size() != static_cast<std::size_t>(gpmp2mi_robot_dof(robot))))
    throw std::runtime_error("[integratePoints] conf does not fit the robot's dof");
  int st[6] = {0, 0, 0, 0, 0, 0};
  check(gpmp2mi_sdf_integrate_points(h, static_cast<int>(points.size() / dim), points.data(), sensor_origin.data(), robot,
                                     robot ? conf->data() : nullptr, margin, &opts, st),
        "gpmp2mi_sdf_integrate_points");
  return EvidenceStatsOf(st);
}
inline std::vector<int16_t> Evidence(const gpmp2mi_sdf* h, std::size_t cells) {
  std::vector<int16_t> e(cells);
  check(gpmp2mi_sdf_get_evidence(h, e.data()), "gpmp2mi_sdf_get_evidence");
  return e;
}
}  // namespace internal

/// Scene (include/gpmp2mi.h "scene"): boxes, spheres, cylinders and closed triangle meshes with poses (row-major 3 x 4
/// [R | t], object -> world).  Objects are added first; the handle is made by the first use (or by build()), after which
/// only poses and enabled flags change.  Only cell centres are tested: give a thin object an inflate of
/// cell * sqrt(3) / 2 to be sure that every cell it touches is marked.
class Scene {
 public:
  using Pose = std::array<double, 12>;
  static Pose identity() { return Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; }
  static Pose translation(double x, double y, double z) { return Pose{1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z}; }
  Scene() = default;
  Scene(const Scene&) = delete;
  Scene& operator=(const Scene&) = delete;
  ~Scene() { gpmp2mi_scene_destroy(h_); }
  /// each returns the index of the new object
  std::size_t addBox(const std::array<double, 3>& half_extents, const Pose& pose, double inflate = 0.0) {
    return add(GPMP2MI_SCENE_BOX, half_extents, inflate, pose, nullptr, nullptr);
  }
  std::size_t addSphere(double radius, const std::array<double, 3>& center, double inflate = 0.0) {
    return add(GPMP2MI_SCENE_SPHERE, {radius, 0.0, 0.0}, inflate, translation(center[0], center[1], center[2]), nullptr,
               nullptr);
  }
  /// axis along the object's z
  std::size_t addCylinder(double radius, double half_height, const Pose& pose, double inflate = 0.0) {
    return add(GPMP2MI_SCENE_CYLINDER, {radius, half_height, 0.0}, inflate, pose, nullptr, nullptr);
  }
  /// a closed mesh: vertices row-major [V][3] in the object frame, triangles [T][3] vertex indices, any winding
  std::size_t addMesh(const Vector& vertices, const std::vector<int>& triangles, const Pose& pose) {
    if (vertices.size() % 3 != 0 || triangles.size() % 3 != 0)
      throw std::runtime_error("[Scene] vertices are not [V][3] or triangles are not [T][3]");
    return add(GPMP2MI_SCENE_MESH, {0.0, 0.0, 0.0}, 0.0, pose, &vertices, &triangles);
  }
  std::size_t size() const { return objs_.size(); }
  void setPose(std::size_t index, const Pose& pose) {
    if (index >= objs_.size()) throw std::runtime_error("[Scene] no such object");
    for (int k = 0; k < 12; k++) objs_[index].pose[k] = pose[k];
    if (h_) check(gpmp2mi_scene_set_poses(h_, static_cast<int>(index), 1, pose.data()), "gpmp2mi_scene_set_poses");
  }
  void setEnabled(std::size_t index, bool enabled) {
    if (index >= objs_.size()) throw std::runtime_error("[Scene] no such object");
    const int e = enabled ? 1 : 0;
    objs_[index].enabled = e;
    if (h_) check(gpmp2mi_scene_set_enabled(h_, static_cast<int>(index), 1, &e), "gpmp2mi_scene_set_enabled");
  }
  /// makes the handle (on the current device) from the objects added so far; no object can be added afterwards
  void build() {
    if (h_) return;
    for (std::size_t k = 0; k < objs_.size(); k++)
      if (objs_[k].kind == GPMP2MI_SCENE_MESH) {
        objs_[k].vertices = verts_[k].data();
        objs_[k].triangles = tris_[k].data();
      }
    check(gpmp2mi_scene_create(static_cast<int>(objs_.size()), objs_.data(), &h_), "gpmp2mi_scene_create");
  }
  const gpmp2mi_scene* handle() {
    build();
    return h_;
  }
  /// the occupied set of the scene alone, one byte per cell [nz][ny][nx]; cells: the count of each object alone
  std::vector<unsigned char> rasterize(const std::array<double, 3>& origin, double cell_size, std::size_t nx,
                                       std::size_t ny, std::size_t nz, std::vector<int>* cells = nullptr) {
    std::vector<unsigned char> mask(nx * ny * nz);
    if (cells) cells->assign(objs_.size(), 0);
    check(gpmp2mi_scene_rasterize(handle(), 3, origin.data(), cell_size, static_cast<int>(nx), static_cast<int>(ny),
                                  static_cast<int>(nz), mask.data(), cells ? cells->data() : nullptr),
          "gpmp2mi_scene_rasterize");
    return mask;
  }

 private:
  std::size_t add(int kind, const std::array<double, 3>& size, double inflate, const Pose& pose, const Vector* vertices,
                  const std::vector<int>* triangles) {
    if (h_) throw std::runtime_error("[Scene] the scene is built: objects can no longer be added");
    gpmp2mi_scene_object o{};
    o.kind = kind;
    for (int k = 0; k < 3; k++) o.size[k] = size[k];
    o.inflate = inflate;
    for (int k = 0; k < 12; k++) o.pose[k] = pose[k];
    o.enabled = 1;
    verts_.push_back(vertices ? *vertices : Vector());
    tris_.push_back(triangles ? *triangles : std::vector<int>());
    o.n_vertices = static_cast<int>(verts_.back().size() / 3);
    o.n_triangles = static_cast<int>(tris_.back().size() / 3);
    objs_.push_back(o);
    return objs_.size() - 1;
  }
  std::vector<gpmp2mi_scene_object> objs_;
  std::vector<Vector> verts_;
  std::vector<std::vector<int>> tris_;
  gpmp2mi_scene* h_ = nullptr;
};

namespace internal {
/// gpmp2mi_sdf_update_from_scene for the two field classes: the cells each object occupies alone
inline std::vector<int> UpdateFieldFromScene(gpmp2mi_sdf* h, Scene& scene, bool use_base, bool use_evidence,
                                             int occupied_at) {
  std::vector<int> cells(scene.size(), 0);
  check(gpmp2mi_sdf_update_from_scene(h, scene.handle(), use_base ? 1 : 0, use_evidence ? 1 : 0, occupied_at,
                                      cells.data()),
        "gpmp2mi_sdf_update_from_scene");
  return cells;
}
}  // namespace internal

/// 3-D signed distance field; data in the reference's own storage order: z slices of column-major
/// (row = y, col = x) matrices, i.e. voxels[(z * cols + x) * rows + y]
class SignedDistanceField {
 public:
  SignedDistanceField(const std::array<double, 3>& origin, double cell_size, std::size_t field_rows,
                      std::size_t field_cols, std::size_t field_z, const Vector& column_major_slices) {
    if (column_major_slices.size() != field_rows * field_cols * field_z)
      throw std::runtime_error("[SignedDistanceField] data size does not match the field dimensions");
    check(gpmp2mi_sdf_create(3, origin.data(), cell_size, static_cast<int>(field_cols), static_cast<int>(field_rows),
                             static_cast<int>(field_z), column_major_slices.data(), GPMP2MI_SDF_LAYOUT_GTSAM, &h_),
          "gpmp2mi_sdf_create");
    cells_ = column_major_slices.size();
  }
  SignedDistanceField(const SignedDistanceField&) = delete;
  SignedDistanceField& operator=(const SignedDistanceField&) = delete;
  ~SignedDistanceField() { gpmp2mi_sdf_destroy(h_); }
  /// getSignedDistance(point, gradient); returns false where the reference throws SDFQueryOutOfRange
  bool getSignedDistance(const std::array<double, 3>& p, double& dist, std::array<double, 3>* grad = nullptr) const {
    int in = 0;
    check(gpmp2mi_sdf_query(h_, 1, p.data(), &dist, grad ? grad->data() : nullptr, &in), "gpmp2mi_sdf_query");
    return in != 0;
  }
  const gpmp2mi_sdf* handle() const { return h_; }
  /// Live map: the field again, in place, from an occupancy grid in the constructor's storage order (cells > 0.75 are
  /// obstacles).  Optimizers already made on this field see the new map in their next call; the grid becomes the base.
  void updateFromOccupancy(const Vector& column_major_slices) {
    if (column_major_slices.size() != cells_)
      throw std::runtime_error("[SignedDistanceField] occupancy size does not match the field dimensions");
    check(gpmp2mi_sdf_update_from_occupancy(h_, column_major_slices.data(), GPMP2MI_SDF_LAYOUT_GTSAM),
          "gpmp2mi_sdf_update_from_occupancy");
  }
  /// Live map: the field again from a point cloud, row-major [M][3], united with the base when use_base
  MapUpdateStats updateFromPoints(const Vector& points, bool use_base = true) {
    return internal::UpdateFieldFromPoints(h_, 3, points, use_base, nullptr, nullptr, 0.0);
  }
  /// ... without the points inside the body spheres of `robot` at `conf`, grown by `margin`
  template <class ROBOT>
  MapUpdateStats updateFromPoints(const Vector& points, bool use_base, const ROBOT& robot, const Vector& conf,
                                  double margin = 0.0) {
    return internal::UpdateFieldFromPoints(h_, 3, points, use_base, robot.handle(), &conf, margin);
  }
  /// Sensor map: one frame of rays from sensor_origin [3] to points (row-major [M][3]) into the evidence kept on this
  /// field -- +hit where a ray ends, -miss where rays pass -- and, with opts.refresh, the field again from the cells
  /// whose evidence reaches opts.occupied_at.  Optimizers already made on this field see the new map in their next call.
  EvidenceStats integratePoints(const Vector& points, const Vector& sensor_origin,
                                const EvidenceOptions& opts = EvidenceOptions()) {
    return internal::IntegratePoints(h_, 3, points, sensor_origin, opts, nullptr, nullptr, 0.0);
  }
  /// ... rays that end inside the body spheres of `robot` at `conf`, grown by `margin`, carve and do not mark
  template <class ROBOT>
  EvidenceStats integratePoints(const Vector& points, const Vector& sensor_origin, const EvidenceOptions& opts,
                                const ROBOT& robot, const Vector& conf, double margin = 0.0) {
    return internal::IntegratePoints(h_, 3, points, sensor_origin, opts, robot.handle(), &conf, margin);
  }
  /// Sensor map: one depth image, row-major [height][width] float metres along the optical axis
  EvidenceStats integrateDepth(const DepthCamera& cam, const std::vector<float>& depth,
                               const EvidenceOptions& opts = EvidenceOptions()) {
    return integrateDepthImpl(cam, depth, opts, nullptr, nullptr, 0.0);
  }
  template <class ROBOT>
  EvidenceStats integrateDepth(const DepthCamera& cam, const std::vector<float>& depth, const EvidenceOptions& opts,
                               const ROBOT& robot, const Vector& conf, double margin = 0.0) {
    if (conf.size() != static_cast<std::size_t>(gpmp2mi_robot_dof(robot.handle())))
      throw std::runtime_error("[integrateDepth] conf does not fit the robot's dof");
    return integrateDepthImpl(cam, depth, opts, robot.handle(), conf.data(), margin);
  }
  /// the field again from the evidence as it stands
  void refreshFromEvidence(int occupied_at = 1, bool use_base = false) {
    check(gpmp2mi_sdf_refresh_from_evidence(h_, occupied_at, use_base ? 1 : 0), "gpmp2mi_sdf_refresh_from_evidence");
  }
  /// the evidence, [z][y][x]
  std::vector<int16_t> evidence() const { return internal::Evidence(h_, cells_); }
  void resetEvidence() { check(gpmp2mi_sdf_evidence_reset(h_), "gpmp2mi_sdf_evidence_reset"); }
  /// Scene: the field again from the enabled objects of `scene`, united with the base (use_base) and with the cells whose
  /// evidence reaches occupied_at (use_evidence).  Returns the cells each object occupies alone (-1: mesh out of range).
  std::vector<int> updateFromScene(Scene& scene, bool use_base = false, bool use_evidence = false, int occupied_at = 1) {
    return internal::UpdateFieldFromScene(h_, scene, use_base, use_evidence, occupied_at);
  }

 private:
  EvidenceStats integrateDepthImpl(const DepthCamera& cam, const std::vector<float>& depth, const EvidenceOptions& opts,
                                   const gpmp2mi_robot* robot, const double* conf, double margin) {
    if (cam.width < 0 || cam.height < 0 ||
        depth.size() != static_cast<std::size_t>(cam.width) * static_cast<std::size_t>(cam.height))
      throw std::runtime_error("[integrateDepth] depth is not [height][width]");
    int st[6] = {0, 0, 0, 0, 0, 0};
    check(gpmp2mi_sdf_integrate_depth(h_, &cam, depth.data(), robot, conf, margin, &opts, st),
          "gpmp2mi_sdf_integrate_depth");
    return internal::EvidenceStatsOf(st);
  }
  gpmp2mi_sdf* h_ = nullptr;
  std::size_t cells_ = 0;
};

/// 2-D signed distance field, column-major (row = y, col = x) like the gtsam::Matrix it replaces
class PlanarSDF {
 public:
  PlanarSDF(const std::array<double, 2>& origin, double cell_size, std::size_t field_rows, std::size_t field_cols,
            const Vector& column_major) {
    if (column_major.size() != field_rows * field_cols)
      throw std::runtime_error("[PlanarSDF] data size does not match the field dimensions");
    const double o[3] = {origin[0], origin[1], 0.0};
    check(gpmp2mi_sdf_create(2, o, cell_size, static_cast<int>(field_cols), static_cast<int>(field_rows), 1,
                             column_major.data(), GPMP2MI_SDF_LAYOUT_GTSAM, &h_),
          "gpmp2mi_sdf_create");
    cells_ = column_major.size();
  }
  PlanarSDF(const PlanarSDF&) = delete;
  PlanarSDF& operator=(const PlanarSDF&) = delete;
  ~PlanarSDF() { gpmp2mi_sdf_destroy(h_); }
  const gpmp2mi_sdf* handle() const { return h_; }
  /// Live map, as SignedDistanceField: occupancy column-major like the constructor's data; points row-major [M][2]
  void updateFromOccupancy(const Vector& column_major) {
    if (column_major.size() != cells_)
      throw std::runtime_error("[PlanarSDF] occupancy size does not match the field dimensions");
    check(gpmp2mi_sdf_update_from_occupancy(h_, column_major.data(), GPMP2MI_SDF_LAYOUT_GTSAM),
          "gpmp2mi_sdf_update_from_occupancy");
  }
  MapUpdateStats updateFromPoints(const Vector& points, bool use_base = true) {
    return internal::UpdateFieldFromPoints(h_, 2, points, use_base, nullptr, nullptr, 0.0);
  }
  template <class ROBOT>
  MapUpdateStats updateFromPoints(const Vector& points, bool use_base, const ROBOT& robot, const Vector& conf,
                                  double margin = 0.0) {
    return internal::UpdateFieldFromPoints(h_, 2, points, use_base, robot.handle(), &conf, margin);
  }
  /// Sensor map, as SignedDistanceField: points row-major [M][2], sensor_origin [2]
  EvidenceStats integratePoints(const Vector& points, const Vector& sensor_origin,
                                const EvidenceOptions& opts = EvidenceOptions()) {
    return internal::IntegratePoints(h_, 2, points, sensor_origin, opts, nullptr, nullptr, 0.0);
  }
  template <class ROBOT>
  EvidenceStats integratePoints(const Vector& points, const Vector& sensor_origin, const EvidenceOptions& opts,
                                const ROBOT& robot, const Vector& conf, double margin = 0.0) {
    return internal::IntegratePoints(h_, 2, points, sensor_origin, opts, robot.handle(), &conf, margin);
  }
  void refreshFromEvidence(int occupied_at = 1, bool use_base = false) {
    check(gpmp2mi_sdf_refresh_from_evidence(h_, occupied_at, use_base ? 1 : 0), "gpmp2mi_sdf_refresh_from_evidence");
  }
  /// the evidence, [y][x]
  std::vector<int16_t> evidence() const { return internal::Evidence(h_, cells_); }
  void resetEvidence() { check(gpmp2mi_sdf_evidence_reset(h_), "gpmp2mi_sdf_evidence_reset"); }
  /// Scene: the field again from the enabled objects of `scene`, united with the base (use_base) and with the cells whose
  /// evidence reaches occupied_at (use_evidence).  Returns the cells each object occupies alone (-1: mesh out of range).
  std::vector<int> updateFromScene(Scene& scene, bool use_base = false, bool use_evidence = false, int occupied_at = 1) {
    return internal::UpdateFieldFromScene(h_, scene, use_base, use_evidence, occupied_at);
  }

 private:
  gpmp2mi_sdf* h_ = nullptr;
  std::size_t cells_ = 0;
};

/// general setting of all trajectory optimizers -- same public fields and setters as the reference
struct TrajOptimizerSetting {
  enum IterationType { GaussNewton = GPMP2MI_OPT_GAUSS_NEWTON, LM = GPMP2MI_OPT_LM, Dogleg = GPMP2MI_OPT_DOGLEG };
  enum VerbosityLevel { None, Error };
  std::size_t dof;
  std::size_t total_step = 10;
  double total_time = 1.0;
  double conf_prior_sigma = 0.0001, vel_prior_sigma = 0.0001;
  bool flag_pos_limit = false, flag_vel_limit = false;
  Vector joint_pos_limits_up, joint_pos_limits_down, vel_limits, pos_limit_thresh, vel_limit_thresh;
  Vector pos_limit_sigmas, vel_limit_sigmas;
  double epsilon = 0.2, cost_sigma = 0.1;
  std::size_t obs_check_inter = 5;
  Vector Qc;  // dof x dof row-major; empty = identity (noiseModel::Unit)
  IterationType opt_type = Dogleg;
  VerbosityLevel opt_verbosity = None;
  bool final_iter_no_increase = true;
  double rel_thresh = 1e-2;
  std::size_t max_iter = 50;

  explicit TrajOptimizerSetting(std::size_t system_dof)
      : dof(system_dof), joint_pos_limits_up(system_dof, 1e6), joint_pos_limits_down(system_dof, -1e6),
        vel_limits(system_dof, 1e6), pos_limit_thresh(system_dof, 0.001), vel_limit_thresh(system_dof, 0.001),
        pos_limit_sigmas(system_dof, 0.001), vel_limit_sigmas(system_dof, 0.001) {}

  void set_total_step(std::size_t step) { total_step = step; }
  void set_total_time(double time) { total_time = time; }
  void set_conf_prior_model(double sigma) { conf_prior_sigma = sigma; }
  void set_vel_prior_model(double sigma) { vel_prior_sigma = sigma; }
  void set_flag_pos_limit(bool flag) { flag_pos_limit = flag; }
  void set_flag_vel_limit(bool flag) { flag_vel_limit = flag; }
  void set_joint_pos_limits_up(const Vector& v) { joint_pos_limits_up = v; }
  void set_joint_pos_limits_down(const Vector& v) { joint_pos_limits_down = v; }
  void set_vel_limits(const Vector& v) { vel_limits = v; }
  void set_pos_limit_thresh(const Vector& v) { pos_limit_thresh = v; }
  void set_vel_limit_thresh(const Vector& v) { vel_limit_thresh = v; }
  void set_pos_limit_model(const Vector& v) { pos_limit_sigmas = v; }
  void set_vel_limit_model(const Vector& v) { vel_limit_sigmas = v; }
  void set_epsilon(double eps) { epsilon = eps; }
  void set_cost_sigma(double sigma) { cost_sigma = sigma; }
  void set_obs_check_inter(std::size_t inter) { obs_check_inter = inter; }
  void set_Qc_model(const Vector& Qc_row_major) { Qc = Qc_row_major; }
  void setGaussNewton() { opt_type = GaussNewton; }
  void setLM() { opt_type = LM; }
  void setDogleg() { opt_type = Dogleg; }
  void set_rel_thresh(double thresh) { rel_thresh = thresh; }
  void set_max_iter(std::size_t iter) { max_iter = iter; }
  void setVerbosityNone() { opt_verbosity = None; }
  void setVerbosityError() { opt_verbosity = Error; }
  void setOptimizationNoIncrase(bool flag) { final_iter_no_increase = flag; }

  gpmp2mi_settings c_struct() const {
    auto fits = [&](const Vector& v, const char* n) {
      if (v.size() != dof) throw std::runtime_error(std::string("[TrajOptimizerSetting] ") + n + " dim does not fit dof");
      return v.data();
    };
    gpmp2mi_settings s;
    gpmp2mi_settings_default(&s, static_cast<int>(dof));
    s.total_step = static_cast<int>(total_step);
    s.total_time = total_time;
    s.conf_prior_sigma = conf_prior_sigma;
    s.vel_prior_sigma = vel_prior_sigma;
    s.flag_pos_limit = flag_pos_limit;
    s.flag_vel_limit = flag_vel_limit;
    s.joint_pos_limits_up = fits(joint_pos_limits_up, "joint_pos_limits_up");
    s.joint_pos_limits_down = fits(joint_pos_limits_down, "joint_pos_limits_down");
    s.vel_limits = fits(vel_limits, "vel_limits");
    s.pos_limit_thresh = fits(pos_limit_thresh, "pos_limit_thresh");
    s.vel_limit_thresh = fits(vel_limit_thresh, "vel_limit_thresh");
    s.pos_limit_sigmas = fits(pos_limit_sigmas, "pos_limit_model");
    s.vel_limit_sigmas = fits(vel_limit_sigmas, "vel_limit_model");
    s.epsilon = epsilon;
    s.cost_sigma = cost_sigma;
    s.obs_check_inter = static_cast<int>(obs_check_inter);
    if (!Qc.empty()) {
      if (Qc.size() != dof * dof) throw std::runtime_error("[TrajOptimizerSetting] Qc dim does not fit dof");
      s.Qc = Qc.data();
    }
    s.opt_type = opt_type;
    s.verbosity = opt_verbosity;
    s.final_iter_no_increase = final_iter_no_increase;
    s.rel_thresh = rel_thresh;
    s.max_iter = static_cast<int>(max_iter);
    return s;
  }
};

/// flat stand-in for gtsam::Values: state(i) = [x_i ; v_i]
struct Trajectory {
  std::size_t dof = 0, total_step = 0;
  Vector data;  // [total_step + 1][2 * dof]
  Trajectory() {}
  Trajectory(std::size_t dof_, std::size_t total_step_) : dof(dof_), total_step(total_step_), data((total_step_ + 1) * 2 * dof_, 0.0) {}
  double* x(std::size_t i) { return &data[i * 2 * dof]; }
  double* v(std::size_t i) { return &data[i * 2 * dof + dof]; }
  const double* x(std::size_t i) const { return &data[i * 2 * dof]; }
  const double* v(std::size_t i) const { return &data[i * 2 * dof + dof]; }
};

/// gpmp2::initArmTrajStraightLine (velocity = (end - init) / total_step, TrajUtils.cpp:45)
inline Trajectory initArmTrajStraightLine(const Vector& init_conf, const Vector& end_conf, std::size_t total_step) {
  const std::size_t D = init_conf.size();
  Trajectory t(D, total_step);
  for (std::size_t i = 0; i <= total_step; i++)
    for (std::size_t k = 0; k < D; k++) {
      const double r = static_cast<double>(i) / static_cast<double>(total_step);
      t.x(i)[k] = (i == 0) ? init_conf[k] : (i == total_step) ? end_conf[k] : r * end_conf[k] + (1.0 - r) * init_conf[k];
      t.v(i)[k] = (end_conf[k] - init_conf[k]) / static_cast<double>(total_step);
    }
  return t;
}

namespace internal {
inline Trajectory BatchTrajOptimize(const gpmp2mi_robot* robot, const gpmp2mi_sdf* sdf, std::size_t dof,
                                    const Vector& start_conf, const Vector& start_vel, const Vector& end_conf,
                                    const Vector& end_vel, const Trajectory& init_values,
                                    const TrajOptimizerSetting& setting, int* iterations, double* final_error) {
  if (init_values.dof != dof || init_values.total_step != setting.total_step)
    throw std::runtime_error("[BatchTrajOptimize] init_values do not match dof / total_step");
  const gpmp2mi_settings s = setting.c_struct();
  Trajectory out(dof, setting.total_step);
  int status = 0;
  check(gpmp2mi_batch_optimize(robot, sdf, &s, nullptr, 1, start_conf.data(), start_vel.data(), end_conf.data(),
                               end_vel.data(), init_values.data.data(), out.data.data(), iterations, final_error,
                               &status),
        "gpmp2mi_batch_optimize");
  if (status == GPMP2MI_TRAJ_NOT_SPD) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
  return out;
}
}  // namespace internal

/// gpmp2::BatchTrajOptimize3DArm  gpmp2/planner/BatchTrajOptimizer.cpp:53-63
inline Trajectory BatchTrajOptimize3DArm(const ArmModel& arm, const SignedDistanceField& sdf, const Vector& start_conf,
                                         const Vector& start_vel, const Vector& end_conf, const Vector& end_vel,
                                         const Trajectory& init_values, const TrajOptimizerSetting& setting,
                                         int* iterations = nullptr, double* final_error = nullptr) {
  return internal::BatchTrajOptimize(arm.handle(), sdf.handle(), arm.dof(), start_conf, start_vel, end_conf, end_vel,
                                     init_values, setting, iterations, final_error);
}
/// gpmp2::BatchTrajOptimize2DArm  gpmp2/planner/BatchTrajOptimizer.cpp:40-50
inline Trajectory BatchTrajOptimize2DArm(const ArmModel& arm, const PlanarSDF& sdf, const Vector& start_conf,
                                         const Vector& start_vel, const Vector& end_conf, const Vector& end_vel,
                                         const Trajectory& init_values, const TrajOptimizerSetting& setting,
                                         int* iterations = nullptr, double* final_error = nullptr) {
  return internal::BatchTrajOptimize(arm.handle(), sdf.handle(), arm.dof(), start_conf, start_vel, end_conf, end_vel,
                                     init_values, setting, iterations, final_error);
}
/// gpmp2::BatchTrajOptimizePose2MobileArm  gpmp2/planner/BatchTrajOptimizer.cpp:79-89
inline Trajectory BatchTrajOptimizePose2MobileArm(const Pose2MobileArmModel& marm, const SignedDistanceField& sdf,
                                                  const Vector& start_conf, const Vector& start_vel, const Vector& end_conf,
                                                  const Vector& end_vel, const Trajectory& init_values,
                                                  const TrajOptimizerSetting& setting, int* iterations = nullptr,
                                                  double* final_error = nullptr) {
  return internal::BatchTrajOptimize(marm.handle(), sdf.handle(), marm.dof(), start_conf, start_vel, end_conf, end_vel,
                                     init_values, setting, iterations, final_error);
}
/// gpmp2::BatchTrajOptimizePose2MobileArm2D  gpmp2/planner/BatchTrajOptimizer.cpp:66-76
inline Trajectory BatchTrajOptimizePose2MobileArm2D(const Pose2MobileArmModel& marm, const PlanarSDF& sdf,
                                                    const Vector& start_conf, const Vector& start_vel,
                                                    const Vector& end_conf, const Vector& end_vel,
                                                    const Trajectory& init_values, const TrajOptimizerSetting& setting,
                                                    int* iterations = nullptr, double* final_error = nullptr) {
  return internal::BatchTrajOptimize(marm.handle(), sdf.handle(), marm.dof(), start_conf, start_vel, end_conf, end_vel,
                                     init_values, setting, iterations, final_error);
}

// ---- factors: evaluateError(x..., H...) of the reference's NoiseModelFactors, one evaluation per call ----------
namespace internal {
template <class ROBOT, class SDF>
class ObstacleSDFFactor {  // gpmp2/obstacle/ObstacleSDFFactor.h:27-100, ObstaclePlanarSDFFactor.h:27-98
 public:
  ObstacleSDFFactor(std::size_t /*poseKey*/, const ROBOT& robot, const SDF& sdf, double /*cost_sigma*/, double epsilon)
      : robot_(robot), sdf_(sdf), epsilon_(epsilon) {}
  /// unwhitened error [nr_body_spheres]; H1 (optional) row-major [nr_body_spheres][dof]
  Vector evaluateError(const Vector& conf, Vector* H1 = nullptr) const {
    if (conf.size() != robot_.dof()) throw std::runtime_error("[ObstacleSDFFactor] conf dim does not fit dof");
    Vector err(robot_.nr_body_spheres());
    if (H1) H1->assign(err.size() * robot_.dof(), 0.0);
    check(gpmp2mi_obstacle_factor(robot_.handle(), sdf_.handle(), epsilon_, 1, conf.data(), err.data(),
                                  H1 ? H1->data() : nullptr),
          "gpmp2mi_obstacle_factor");
    return err;
  }

 private:
  const ROBOT& robot_;
  const SDF& sdf_;
  double epsilon_;
};
}  // namespace internal
typedef internal::ObstacleSDFFactor<ArmModel, SignedDistanceField> ObstacleSDFFactorArm;
typedef internal::ObstacleSDFFactor<ArmModel, PlanarSDF> ObstaclePlanarSDFFactorArm;
typedef internal::ObstacleSDFFactor<Pose2MobileArmModel, SignedDistanceField> ObstacleSDFFactorPose2MobileArm;
typedef internal::ObstacleSDFFactor<Pose2MobileArmModel, PlanarSDF> ObstaclePlanarSDFFactorPose2MobileArm;

/// gpmp2::GoalFactorArm  gpmp2/kinematics/GoalFactorArm.h:24-100
class GoalFactorArm {
 public:
  GoalFactorArm(std::size_t /*poseKey*/, const ArmModel& arm, const std::array<double, 3>& dest_point)
      : arm_(arm), dest_(dest_point) {}
  Vector evaluateError(const Vector& conf, Vector* H1 = nullptr) const {
    Vector err(3);
    if (H1) H1->assign(3 * arm_.dof(), 0.0);
    check(gpmp2mi_goal_factor_arm(arm_.handle(), dest_.data(), 1, conf.data(), err.data(), H1 ? H1->data() : nullptr),
          "gpmp2mi_goal_factor_arm");
    return err;
  }

 private:
  const ArmModel& arm_;
  std::array<double, 3> dest_;
};

/// gpmp2::GaussianPriorWorkspacePoseArm  gpmp2/kinematics/GaussianPriorWorkspacePose.h:24-93
class GaussianPriorWorkspacePoseArm {
 public:
  GaussianPriorWorkspacePoseArm(std::size_t /*poseKey*/, const ArmModel& arm, int joint, const Pose3& des_pose)
      : arm_(arm), joint_(joint), des_(des_pose) {}
  Vector evaluateError(const Vector& conf, Vector* H1 = nullptr) const {
    Vector err(6);
    if (H1) H1->assign(6 * arm_.dof(), 0.0);
    check(gpmp2mi_workspace_prior_factor(arm_.handle(), GPMP2MI_WORKSPACE_POSE, joint_, des_.m.data(), 1, conf.data(),
                                         err.data(), H1 ? H1->data() : nullptr),
          "gpmp2mi_workspace_prior_factor");
    return err;
  }

 private:
  const ArmModel& arm_;
  int joint_;
  Pose3 des_;
};

/// gpmp2::SelfCollisionArm  gpmp2/obstacle/SelfCollision.h:27-140; data rows = (sphere A, sphere B, epsilon, sigma)
class SelfCollisionArm {
 public:
  SelfCollisionArm(std::size_t /*poseKey*/, const ArmModel& arm, const Vector& data_row_major) : arm_(arm), data_(data_row_major) {
    if (data_.size() % 4) throw std::runtime_error("[SelfCollision] data must have 4 columns");
  }
  Vector evaluateError(const Vector& conf, Vector* H = nullptr) const {
    const int np = static_cast<int>(data_.size() / 4);
    Vector err(np);
    if (H) H->assign(np * arm_.dof(), 0.0);
    check(gpmp2mi_self_collision_factor(arm_.handle(), np, data_.data(), 1, conf.data(), err.data(), H ? H->data() : nullptr),
          "gpmp2mi_self_collision_factor");
    return err;
  }

 private:
  const ArmModel& arm_;
  Vector data_;
};

/// gpmp2::CollisionCost3DArm / 2DArm  gpmp2/planner/BatchTrajOptimizer-inl.h:87-100
inline double CollisionCost3DArm(const ArmModel& arm, const SignedDistanceField& sdf, const Trajectory& result,
                                 const TrajOptimizerSetting&) {
  double c = 0;
  check(gpmp2mi_collision_cost(arm.handle(), sdf.handle(), static_cast<int>(result.total_step), 1, result.data.data(), &c),
        "gpmp2mi_collision_cost");
  return c;
}
inline double CollisionCost2DArm(const ArmModel& arm, const PlanarSDF& sdf, const Trajectory& result,
                                 const TrajOptimizerSetting&) {
  double c = 0;
  check(gpmp2mi_collision_cost(arm.handle(), sdf.handle(), static_cast<int>(result.total_step), 1, result.data.data(), &c),
        "gpmp2mi_collision_cost");
  return c;
}

/// What the executed trajectory looks like to the obstacles (include/gpmp2mi.h "scoring"): the collision cost of the
/// support states (= CollisionCost*), the same sum over the trajectory up-sampled with inter_step states per interval
/// (the states interpolateArmTraj hands to the controller), the smallest signed clearance with the checked state and
/// sphere where it occurs ((-1, -1) and +inf when no sphere centre is inside the field) and the number of
/// (state, sphere) pairs outside the field.
struct TrajectoryScore {
  double support_cost = 0.0, dense_cost = 0.0, min_clearance = 0.0;
  int worst_state = -1, worst_sphere = -1, out_of_range = 0;
};
/// ROBOT: any of the robot models; SDF: SignedDistanceField or PlanarSDF.  delta_t = total_time / total_step.
template <class ROBOT, class SDF>
inline TrajectoryScore ScoreTrajectory(const ROBOT& robot, const SDF& sdf, const Trajectory& result,
                                       const TrajOptimizerSetting& setting, std::size_t inter_step) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[ScoreTrajectory] result does not match dof / total_step");
  TrajectoryScore sc;
  int worst[2] = {-1, -1};
  check(gpmp2mi_score_traj(robot.handle(), sdf.handle(), setting.total_time / static_cast<double>(setting.total_step),
                           static_cast<int>(inter_step), 1, static_cast<int>(result.total_step), result.data.data(),
                           &sc.support_cost, &sc.dense_cost, &sc.min_clearance, worst, &sc.out_of_range),
        "gpmp2mi_score_traj");
  sc.worst_state = worst[0];
  sc.worst_sphere = worst[1];
  return sc;
}
/// Best of several results (restarts): the index of the eligible one with the smallest final_error, the lowest index
/// on ties, -1 if none is eligible.  Eligible: status != GPMP2MI_TRAJ_NOT_SPD (status may be empty: all fine), finite
/// final_error, min_clearance >= required_clearance and, with require_in_range, no pair outside the field.  Host code.
inline int SelectBestTrajectory(const Vector& final_error, const std::vector<int>& status,
                                const std::vector<TrajectoryScore>& scores, double required_clearance = 0.0,
                                bool require_in_range = false, std::size_t* n_eligible = nullptr) {
  if (scores.size() != final_error.size() || (!status.empty() && status.size() != final_error.size()))
    throw std::runtime_error("[SelectBestTrajectory] final_error, status and scores differ in length");
  Vector clearance(scores.size());
  std::vector<int> oor(scores.size());
  for (std::size_t b = 0; b < scores.size(); b++) {
    clearance[b] = scores[b].min_clearance;
    oor[b] = scores[b].out_of_range;
  }
  int best = -1, n = 0;
  check(gpmp2mi_select_best(static_cast<int>(scores.size()), final_error.data(), status.empty() ? nullptr : status.data(),
                            clearance.data(), oor.data(), required_clearance, require_in_range ? 1 : 0, &best, &n),
        "gpmp2mi_select_best");
  if (n_eligible) *n_eligible = static_cast<std::size_t>(n);
  return best;
}

/// A pair table of the self-collision check (include/gpmp2mi.h "self-collision check"), resident on the device and bound
/// to the sphere model of `robot`: rows (sphere A, sphere B, epsilon, sigma) as gpmp2::SelfCollision takes them, or
/// generated from the robot's kinematic tree (all pairs at least min_joint_gap joints apart, less those that overlap at
/// a reference configuration).  Move-only.
class SelfCollisionPairs {
 public:
  template <class ROBOT>
  SelfCollisionPairs(const ROBOT& robot, const Vector& data_row_major) {
    if (data_row_major.size() % 4) throw std::runtime_error("[SelfCollisionPairs] data must have 4 columns");
    check(gpmp2mi_self_pairs_create(robot.handle(), static_cast<int>(data_row_major.size() / 4), data_row_major.data(), &h_),
          "gpmp2mi_self_pairs_create");
  }
  /// ref_conf: n reference configurations back to back (may be empty)
  template <class ROBOT>
  static SelfCollisionPairs Generate(const ROBOT& robot, int min_joint_gap = 2, const Vector& ref_conf = {},
                                     double epsilon = 0.0, double sigma = 1.0) {
    if (ref_conf.size() % robot.dof()) throw std::runtime_error("[SelfCollisionPairs] ref_conf does not fit the dof");
    SelfCollisionPairs t;
    check(gpmp2mi_self_pairs_generate(robot.handle(), min_joint_gap, static_cast<int>(ref_conf.size() / robot.dof()),
                                      ref_conf.empty() ? nullptr : ref_conf.data(), epsilon, sigma, &t.h_),
          "gpmp2mi_self_pairs_generate");
    return t;
  }
  SelfCollisionPairs(SelfCollisionPairs&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  SelfCollisionPairs& operator=(SelfCollisionPairs&& o) noexcept {
    if (this != &o) {
      gpmp2mi_self_pairs_destroy(h_);
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  SelfCollisionPairs(const SelfCollisionPairs&) = delete;
  SelfCollisionPairs& operator=(const SelfCollisionPairs&) = delete;
  ~SelfCollisionPairs() { gpmp2mi_self_pairs_destroy(h_); }
  std::size_t size() const { return static_cast<std::size_t>(gpmp2mi_self_pairs_count(h_)); }
  /// the rows, [size()][4] row-major
  Vector data() const {
    Vector d(size() * 4);
    check(gpmp2mi_self_pairs_get(h_, d.data()), "gpmp2mi_self_pairs_get");
    return d;
  }
  const gpmp2mi_self_pairs* handle() const { return h_; }

 private:
  SelfCollisionPairs() = default;
  gpmp2mi_self_pairs* h_ = nullptr;
};

/// What the executed trajectory looks like to the robot itself: the SelfCollision hinge summed over the support states
/// and over the up-sampled states, the smallest pair clearance with the checked state and table row where it occurs
/// ((-1, -1) and +inf for an empty table) and the number of (state, pair)s whose distance is not finite.
struct TrajectorySelfScore {
  double support_cost = 0.0, dense_cost = 0.0, min_clearance = 0.0;
  int worst_state = -1, worst_pair = -1, invalid = 0;
};
template <class ROBOT>
inline TrajectorySelfScore SelfScoreTrajectory(const ROBOT& robot, const SelfCollisionPairs& pairs, const Trajectory& result,
                                               const TrajOptimizerSetting& setting, std::size_t inter_step) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[SelfScoreTrajectory] result does not match dof / total_step");
  TrajectorySelfScore sc;
  int worst[2] = {-1, -1};
  check(gpmp2mi_self_score_traj(robot.handle(), pairs.handle(), setting.total_time / static_cast<double>(setting.total_step),
                                static_cast<int>(inter_step), 1, static_cast<int>(result.total_step), result.data.data(),
                                &sc.support_cost, &sc.dense_cost, &sc.min_clearance, worst, &sc.invalid),
        "gpmp2mi_self_score_traj");
  sc.worst_state = worst[0];
  sc.worst_pair = worst[1];
  return sc;
}
/// SelectBestTrajectory that also looks at the robot itself: a result is eligible when the SMALLER of its two clearances
/// (obstacles, itself) reaches required_clearance and none of its pairs is invalid; the rest as above.  Host code.
inline int SelectBestTrajectory(const Vector& final_error, const std::vector<int>& status,
                                const std::vector<TrajectoryScore>& scores, const std::vector<TrajectorySelfScore>& self_scores,
                                double required_clearance = 0.0, bool require_in_range = false,
                                std::size_t* n_eligible = nullptr) {
  if (self_scores.size() != scores.size())
    throw std::runtime_error("[SelectBestTrajectory] scores and self_scores differ in length");
  std::vector<TrajectoryScore> both(scores);
  for (std::size_t b = 0; b < both.size(); b++) {
    // std::min keeps a NaN first argument, and a NaN clearance is never eligible
    both[b].min_clearance = self_scores[b].invalid != 0 ? std::nan("") : std::min(scores[b].min_clearance, self_scores[b].min_clearance);
    if (self_scores[b].min_clearance != self_scores[b].min_clearance) both[b].min_clearance = std::nan("");
  }
  return SelectBestTrajectory(final_error, status, both, required_clearance, require_in_range, n_eligible);
}

/// The motion limits of a robot (include/gpmp2mi.h "motion limits"): joint ranges, joint speeds, joint accelerations,
/// each empty (no limit of that kind) or one entry per coordinate with +-infinity where a coordinate has none, and the
/// Cartesian speed limit of the body spheres (infinity: none).
struct MotionLimits {
  Vector pos_down, pos_up, vel, acc;
  double point_speed = std::numeric_limits<double>::infinity();
  /// the C struct over this object's arrays: valid while the object lives and is not modified
  gpmp2mi_motion_limits c(std::size_t dof) const {
    for (const Vector* v : {&pos_down, &pos_up, &vel, &acc})
      if (!v->empty() && v->size() != dof) throw std::runtime_error("[MotionLimits] an array does not fit the dof");
    gpmp2mi_motion_limits l;
    l.pos_down = pos_down.empty() ? nullptr : pos_down.data();
    l.pos_up = pos_up.empty() ? nullptr : pos_up.data();
    l.vel = vel.empty() ? nullptr : vel.data();
    l.acc = acc.empty() ? nullptr : acc.data();
    l.point_speed = point_speed;
    return l;
  }
};
/// Whether the robot can execute the up-sampled trajectory: the smallest distance to a joint range (negative: outside),
/// the largest joint speed and joint acceleration relative to their limits, the largest speed of a sphere centre, each
/// with where it occurs ((-1, -1) if nothing is limited), the factor by which the duration must be stretched to meet
/// every rate limit (<= 1: executable as planned) and the number of quantities that are not finite.
struct TrajectoryMotionScore {
  double pos_margin = 0.0, vel_ratio = 0.0, acc_ratio = 0.0, point_speed = 0.0, time_scale = 0.0;
  int pos_state = -1, pos_coord = -1, vel_state = -1, vel_coord = -1, acc_end = -1, acc_coord = -1, speed_state = -1,
      speed_sphere = -1, invalid = 0;
};
template <class ROBOT>
inline TrajectoryMotionScore MotionScoreTrajectory(const ROBOT& robot, const MotionLimits& limits, const Trajectory& result,
                                                   const TrajOptimizerSetting& setting, std::size_t inter_step) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[MotionScoreTrajectory] result does not match dof / total_step");
  const gpmp2mi_motion_limits l = limits.c(robot.dof());
  TrajectoryMotionScore sc;
  int worst[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  check(gpmp2mi_motion_score_traj(robot.handle(), &l, setting.total_time / static_cast<double>(setting.total_step),
                                  static_cast<int>(inter_step), 1, static_cast<int>(result.total_step), result.data.data(),
                                  &sc.pos_margin, &sc.vel_ratio, &sc.acc_ratio, &sc.point_speed, &sc.time_scale, worst,
                                  &sc.invalid),
        "gpmp2mi_motion_score_traj");
  sc.pos_state = worst[0]; sc.pos_coord = worst[1]; sc.vel_state = worst[2]; sc.vel_coord = worst[3];
  sc.acc_end = worst[4]; sc.acc_coord = worst[5]; sc.speed_state = worst[6]; sc.speed_sphere = worst[7];
  return sc;
}
/// SelectBestTrajectory that also asks whether the robot can execute the result: besides the rule above, no motion
/// quantity may be non-finite, pos_margin must reach required_pos_margin and time_scale must not exceed max_time_scale.
/// Host code.
inline int SelectBestTrajectory(const Vector& final_error, const std::vector<int>& status,
                                const std::vector<TrajectoryScore>& scores,
                                const std::vector<TrajectoryMotionScore>& motion_scores, double required_pos_margin,
                                double max_time_scale, double required_clearance = 0.0, bool require_in_range = false,
                                std::size_t* n_eligible = nullptr) {
  if (motion_scores.size() != scores.size())
    throw std::runtime_error("[SelectBestTrajectory] scores and motion_scores differ in length");
  if (required_pos_margin != required_pos_margin || max_time_scale != max_time_scale)
    throw std::runtime_error("[SelectBestTrajectory] required_pos_margin / max_time_scale is NaN");
  std::vector<TrajectoryScore> both(scores);
  for (std::size_t b = 0; b < both.size(); b++) {
    const TrajectoryMotionScore& m = motion_scores[b];
    const bool ok = m.invalid == 0 && m.pos_margin >= required_pos_margin && m.time_scale <= max_time_scale;
    if (!ok) both[b].min_clearance = std::nan("");   // a NaN clearance is never eligible
  }
  return SelectBestTrajectory(final_error, status, both, required_clearance, require_in_range, n_eligible);
}

/// The speed profile of a trajectory along its unchanged path (include/gpmp2mi.h "re-timing"): at every checked state k
/// the rate sdot[k] of planned against executed time, the path acceleration u[k] of the stage behind it and the new time
/// stamp stamps[k], such that the duration is as short as the rate limits (vel, acc, point_speed of MotionLimits; the
/// joint ranges are not read) and max_rate allow.  status is GPMP2MI_RETIME_OK or says why there is no profile (then
/// duration is +infinity and the arrays hold NaN).  achieved: the largest velocity, stage-end acceleration, stage-midpoint
/// acceleration and point-speed ratios after re-timing.  dense holds the checked states with their velocities multiplied
/// by sdot.  The moving-obstacle and workspace-path checks of a trajectory index by planned time: they do not hold for
/// the re-timed one.
struct RetimedTrajectory {
  Vector sdot, u, stamps;
  double duration = 0.0, achieved[4] = {0.0, 0.0, 0.0, 0.0};
  int status = GPMP2MI_RETIME_INVALID;
  Trajectory dense;   // total_step * (inter_step + 1) intervals
};
/// ROBOT: a fixed-base robot model (the Pose2 kinds throw).  rate_start / rate_end: a forced rate at the first / last
/// state (0: at rest), negative: free.  With max_rate = 1 the robot never runs faster than planned.
template <class ROBOT>
inline RetimedTrajectory RetimeTrajectory(const ROBOT& robot, const MotionLimits& limits, const Trajectory& result,
                                          const TrajOptimizerSetting& setting, std::size_t inter_step, double max_rate = 1.0,
                                          double rate_start = -1.0, double rate_end = -1.0) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[RetimeTrajectory] result does not match dof / total_step");
  const gpmp2mi_motion_limits l = limits.c(robot.dof());
  RetimedTrajectory rt;
  rt.dense = Trajectory(result.dof, result.total_step * (inter_step + 1));
  const std::size_t Md = rt.dense.total_step + 1;
  rt.sdot.assign(Md, 0.0);
  rt.u.assign(Md, 0.0);
  rt.stamps.assign(Md, 0.0);
  check(gpmp2mi_retime_traj(robot.handle(), &l, setting.total_time / static_cast<double>(setting.total_step),
                            static_cast<int>(inter_step), 1, static_cast<int>(result.total_step), result.data.data(), max_rate,
                            rate_start, rate_end, rt.sdot.data(), rt.u.data(), rt.stamps.data(), &rt.duration, &rt.status,
                            rt.achieved, rt.dense.data.data()),
        "gpmp2mi_retime_traj");
  return rt;
}
/// The SelectBestTrajectory above with the duration of the re-timed result in place of time_scale: besides the rule of
/// the obstacle scores, no motion quantity may be non-finite, pos_margin must reach required_pos_margin, and the result
/// must re-time (GPMP2MI_RETIME_OK) within max_duration.  Host code.
inline int SelectBestTrajectory(const Vector& final_error, const std::vector<int>& status,
                                const std::vector<TrajectoryScore>& scores,
                                const std::vector<TrajectoryMotionScore>& motion_scores,
                                const std::vector<RetimedTrajectory>& retimed, double required_pos_margin, double max_duration,
                                double required_clearance = 0.0, bool require_in_range = false,
                                std::size_t* n_eligible = nullptr) {
  if (motion_scores.size() != scores.size() || retimed.size() != scores.size())
    throw std::runtime_error("[SelectBestTrajectory] scores, motion_scores and retimed differ in length");
  if (required_pos_margin != required_pos_margin || max_duration != max_duration)
    throw std::runtime_error("[SelectBestTrajectory] required_pos_margin / max_duration is NaN");
  std::vector<TrajectoryScore> both(scores);
  for (std::size_t b = 0; b < both.size(); b++) {
    const TrajectoryMotionScore& m = motion_scores[b];
    const bool ok = m.invalid == 0 && m.pos_margin >= required_pos_margin && retimed[b].status == GPMP2MI_RETIME_OK &&
                    retimed[b].duration <= max_duration;
    if (!ok) both[b].min_clearance = std::nan("");   // a NaN clearance is never eligible
  }
  return SelectBestTrajectory(final_error, status, both, required_clearance, require_in_range, n_eligible);
}

/// The inertial table of a fixed-base arm on the device (include/gpmp2mi.h "torque limits"), bound to the kinematics of
/// the robot it was made for: mass [L], com [L][3] in the link frames, inertia [L][6] = ixx iyy izz ixy ixz iyz about the
/// centres of mass, gravity in the world frame, and the torque limits [dof] (empty: none; +infinity: none for that joint).
/// ROBOT: a fixed-base arm of at most 8 joints (anything else throws, the reason in the message).
class ArmDynamics {
 public:
  template <class ROBOT>
  ArmDynamics(const ROBOT& robot, const Vector& mass, const Vector& com, const Vector& inertia, const Vector& torque = {},
              const std::array<double, 3>& gravity = {0.0, 0.0, -9.81}) {
    const std::size_t L = static_cast<std::size_t>(gpmp2mi_robot_nr_links(robot.handle()));
    if (mass.size() != L || com.size() != 3 * L || inertia.size() != 6 * L)
      throw std::runtime_error("[ArmDynamics] mass / com / inertia do not fit the number of links");
    if (!torque.empty() && torque.size() != robot.dof()) throw std::runtime_error("[ArmDynamics] torque does not fit the dof");
    gpmp2mi_dynamics_desc d;
    gpmp2mi_dynamics_desc_default(&d);
    d.mass = mass.data();
    d.com = com.data();
    d.inertia = inertia.data();
    d.torque = torque.empty() ? nullptr : torque.data();
    for (int i = 0; i < 3; i++) d.gravity[i] = gravity[i];
    check(gpmp2mi_dynamics_create(robot.handle(), &d, &h_), "gpmp2mi_dynamics_create");
  }
  ArmDynamics(ArmDynamics&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ArmDynamics& operator=(ArmDynamics&& o) noexcept {
    if (this != &o) {
      gpmp2mi_dynamics_destroy(h_);
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ArmDynamics(const ArmDynamics&) = delete;
  ArmDynamics& operator=(const ArmDynamics&) = delete;
  ~ArmDynamics() { gpmp2mi_dynamics_destroy(h_); }
  const gpmp2mi_dynamics* handle() const { return h_; }

 private:
  gpmp2mi_dynamics* h_ = nullptr;
};
/// Whether the drives can produce the up-sampled trajectory: the largest joint torque and the largest gravity torque
/// relative to their limits, the factor by which the duration must be stretched to meet every torque limit (<= 1: as
/// planned; +infinity: gravity alone is too much), each with the (state, joint) where it occurs ((-1, -1) if nothing is
/// limited), the number of torques that are not finite, and the torques themselves, [Md][dof] at planned timing (the
/// feed-forward term).  The torque between checked states is sampled, not bounded.
struct TrajectoryTorqueScore {
  double torque_ratio = 0.0, static_ratio = 0.0, time_scale = 0.0;
  int torque_state = -1, torque_joint = -1, static_state = -1, static_joint = -1, scale_state = -1, scale_joint = -1,
      invalid = 0;
  Vector tau;
};
template <class ROBOT>
inline TrajectoryTorqueScore TorqueScore(const ROBOT& robot, const ArmDynamics& dynamics, const Trajectory& result,
                                         const TrajOptimizerSetting& setting, std::size_t inter_step) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[TorqueScore] result does not match dof / total_step");
  TrajectoryTorqueScore sc;
  sc.tau.assign((result.total_step * (inter_step + 1) + 1) * result.dof, 0.0);
  int worst[6] = {-1, -1, -1, -1, -1, -1};
  check(gpmp2mi_torque_score_traj(robot.handle(), dynamics.handle(), setting.total_time / static_cast<double>(setting.total_step),
                                  static_cast<int>(inter_step), 1, static_cast<int>(result.total_step), result.data.data(),
                                  &sc.torque_ratio, &sc.static_ratio, &sc.time_scale, worst, &sc.invalid, sc.tau.data()),
        "gpmp2mi_torque_score_traj");
  sc.torque_state = worst[0]; sc.torque_joint = worst[1]; sc.static_state = worst[2]; sc.static_joint = worst[3];
  sc.scale_state = worst[4]; sc.scale_joint = worst[5];
  return sc;
}
/// The SelectBestTrajectory of the motion scores with the torques: the LARGER of the two stretches (motion limits, torque
/// limits) must not exceed max_time_scale, and no torque may be non-finite.  Host code.
inline int SelectBestTrajectory(const Vector& final_error, const std::vector<int>& status,
                                const std::vector<TrajectoryScore>& scores,
                                const std::vector<TrajectoryMotionScore>& motion_scores,
                                const std::vector<TrajectoryTorqueScore>& torque_scores, double required_pos_margin,
                                double max_time_scale, double required_clearance = 0.0, bool require_in_range = false,
                                std::size_t* n_eligible = nullptr) {
  if (motion_scores.size() != scores.size() || torque_scores.size() != scores.size())
    throw std::runtime_error("[SelectBestTrajectory] scores, motion_scores and torque_scores differ in length");
  if (required_pos_margin != required_pos_margin || max_time_scale != max_time_scale)
    throw std::runtime_error("[SelectBestTrajectory] required_pos_margin / max_time_scale is NaN");
  std::vector<TrajectoryScore> both(scores);
  for (std::size_t b = 0; b < both.size(); b++) {
    const TrajectoryMotionScore& m = motion_scores[b];
    const TrajectoryTorqueScore& t = torque_scores[b];
    const double scale = t.time_scale > m.time_scale ? t.time_scale : m.time_scale;
    const bool ok = m.invalid == 0 && t.invalid == 0 && m.pos_margin >= required_pos_margin && scale <= max_time_scale;
    if (!ok) both[b].min_clearance = std::nan("");   // a NaN clearance is never eligible
  }
  return SelectBestTrajectory(final_error, status, both, required_clearance, require_in_range, n_eligible);
}

/// The speed profile of a trajectory under the joint torque limits of an ArmDynamics, next to the rate limits of
/// RetimeTrajectory (include/gpmp2mi.h "re-timing under torque limits"): the members of RetimedTrajectory, with two more
/// entries of achieved (the largest torque ratio of the re-timed result at its checked states, <= 1 up to rounding, and
/// the largest share gravity alone takes of a limit), the torques the re-timed result asks for, tau [Md][dof] (the
/// feed-forward term), and the coefficients coef [Md][4][dof] = p, m_left, m_right, tau_g of tau = p u + m sdot^2 + tau_g.
/// status may also be GPMP2MI_RETIME_STATIC: gravity alone exceeds a limit, no timing helps.  The torque between checked
/// states is sampled, not bounded.
struct DynamicRetimedTrajectory {
  Vector sdot, u, stamps;
  double duration = 0.0, achieved[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int status = GPMP2MI_RETIME_INVALID;
  Trajectory dense;   // total_step * (inter_step + 1) intervals
  Vector tau, coef;
};
/// ROBOT: a fixed-base arm of at most 8 joints (anything else throws, the reason in the message).
template <class ROBOT>
inline DynamicRetimedTrajectory RetimeTrajectory(const ROBOT& robot, const ArmDynamics& dynamics, const MotionLimits& limits,
                                                 const Trajectory& result, const TrajOptimizerSetting& setting,
                                                 std::size_t inter_step, double max_rate = 1.0, double rate_start = -1.0,
                                                 double rate_end = -1.0) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[RetimeTrajectory] result does not match dof / total_step");
  const gpmp2mi_motion_limits l = limits.c(robot.dof());
  DynamicRetimedTrajectory rt;
  rt.dense = Trajectory(result.dof, result.total_step * (inter_step + 1));
  const std::size_t Md = rt.dense.total_step + 1;
  rt.sdot.assign(Md, 0.0);
  rt.u.assign(Md, 0.0);
  rt.stamps.assign(Md, 0.0);
  rt.tau.assign(Md * result.dof, 0.0);
  rt.coef.assign(Md * 4 * result.dof, 0.0);
  check(gpmp2mi_retime_dynamic_traj(robot.handle(), dynamics.handle(), &l,
                                    setting.total_time / static_cast<double>(setting.total_step), static_cast<int>(inter_step),
                                    1, static_cast<int>(result.total_step), result.data.data(), max_rate, rate_start, rate_end,
                                    rt.sdot.data(), rt.u.data(), rt.stamps.data(), &rt.duration, &rt.status, rt.achieved,
                                    rt.dense.data.data(), rt.tau.data(), rt.coef.data()),
        "gpmp2mi_retime_dynamic_traj");
  return rt;
}
/// The SelectBestTrajectory of the re-timed results, with the torque rows in the profile: the result must re-time
/// (GPMP2MI_RETIME_OK) within max_duration, and none of its coefficients may be non-finite.  Host code.
inline int SelectBestTrajectory(const Vector& final_error, const std::vector<int>& status,
                                const std::vector<TrajectoryScore>& scores,
                                const std::vector<TrajectoryMotionScore>& motion_scores,
                                const std::vector<DynamicRetimedTrajectory>& retimed, double required_pos_margin,
                                double max_duration, double required_clearance = 0.0, bool require_in_range = false,
                                std::size_t* n_eligible = nullptr) {
  if (motion_scores.size() != scores.size() || retimed.size() != scores.size())
    throw std::runtime_error("[SelectBestTrajectory] scores, motion_scores and retimed differ in length");
  if (required_pos_margin != required_pos_margin || max_duration != max_duration)
    throw std::runtime_error("[SelectBestTrajectory] required_pos_margin / max_duration is NaN");
  std::vector<TrajectoryScore> both(scores);
  for (std::size_t b = 0; b < both.size(); b++) {
    const TrajectoryMotionScore& m = motion_scores[b];
    bool ok = m.invalid == 0 && m.pos_margin >= required_pos_margin && retimed[b].status == GPMP2MI_RETIME_OK &&
              retimed[b].duration <= max_duration;
    for (double c : retimed[b].coef) ok = ok && std::isfinite(c);
    if (!ok) both[b].min_clearance = std::nan("");   // a NaN clearance is never eligible
  }
  return SelectBestTrajectory(final_error, status, both, required_clearance, require_in_range, n_eligible);
}

namespace internal {
inline Trajectory interpolateTraj(const Trajectory& opt_values, const Vector& Qc, double delta_t, std::size_t inter_step,
                                  std::size_t start_index, std::size_t end_index, bool lie) {
  if (!Qc.empty() && Qc.size() != opt_values.dof * opt_values.dof)
    throw std::runtime_error("[interpolateArmTraj] Qc dim does not fit dof");
  if (start_index >= end_index || end_index > opt_values.total_step)
    throw std::runtime_error("[interpolateArmTraj] need start_index < end_index <= total_step");
  Trajectory out(opt_values.dof, (end_index - start_index) * (inter_step + 1));
  check(gpmp2mi_interpolate_traj(static_cast<int>(opt_values.dof), lie ? 1 : 0, Qc.empty() ? nullptr : Qc.data(), delta_t,
                                 static_cast<int>(inter_step), 1, static_cast<int>(opt_values.total_step),
                                 static_cast<int>(start_index), static_cast<int>(end_index), opt_values.data.data(),
                                 out.data.data()),
        "gpmp2mi_interpolate_traj");
  return out;
}
}  // namespace internal
/// gpmp2::interpolateArmTraj  gpmp2/planner/TrajUtils.cpp:96-159 (Qc row-major [dof][dof], may be empty)
inline Trajectory interpolateArmTraj(const Trajectory& opt_values, const Vector& Qc, double delta_t, std::size_t inter_step) {
  return internal::interpolateTraj(opt_values, Qc, delta_t, inter_step, 0, opt_values.total_step, false);
}
/// gpmp2::interpolateArmTraj with a state range  gpmp2/planner/TrajUtils.cpp:162-197
inline Trajectory interpolateArmTraj(const Trajectory& opt_values, const Vector& Qc, double delta_t, std::size_t inter_step,
                                     std::size_t start_index, std::size_t end_index) {
  return internal::interpolateTraj(opt_values, Qc, delta_t, inter_step, start_index, end_index, false);
}
/// gpmp2::interpolatePose2MobileArmTraj  gpmp2/planner/TrajUtils.cpp:200-236 (states [x, y, theta, q...])
inline Trajectory interpolatePose2MobileArmTraj(const Trajectory& opt_values, const Vector& Qc, double delta_t,
                                                std::size_t inter_step, std::size_t start_index, std::size_t end_index) {
  return internal::interpolateTraj(opt_values, Qc, delta_t, inter_step, start_index, end_index, true);
}

namespace internal {
/// gpmp2::internal::ISAM2TrajOptimizer  gpmp2/planner/ISAM2TrajOptimizer.h:58-137
/// Same call sequence as the reference (initFactorGraph, initValues, update, then the replanning
/// interface and update again); each update() is one full relinearise + solve of the resident plan
/// (gpmp2mi_plan_update), not an iSAM2 partial update -- see include/gpmp2mi.h.
template <class ROBOT, class SDF>
class ISAM2TrajOptimizer {
 public:
  ISAM2TrajOptimizer(const ROBOT& arm, const SDF& sdf, const TrajOptimizerSetting& setting)
      : dof_(arm.dof()), setting_(setting) {
    const gpmp2mi_settings s = setting_.c_struct();
    check(gpmp2mi_plan_create(arm.handle(), sdf.handle(), &s, nullptr, 1, &plan_), "gpmp2mi_plan_create");
  }
  ~ISAM2TrajOptimizer() {
    if (plan_) gpmp2mi_plan_destroy(plan_);
  }
  ISAM2TrajOptimizer(const ISAM2TrajOptimizer&) = delete;
  ISAM2TrajOptimizer& operator=(const ISAM2TrajOptimizer&) = delete;

  /// ISAM2TrajOptimizer-inl.h:28-84
  void initFactorGraph(const Vector& start_conf, const Vector& start_vel, const Vector& goal_conf, const Vector& goal_vel) {
    start_conf_ = start_conf, start_vel_ = start_vel, goal_conf_ = goal_conf, goal_vel_ = goal_vel;
    fits(start_conf), fits(start_vel), fits(goal_conf), fits(goal_vel);
    have_graph_ = true;
  }
  /// ISAM2TrajOptimizer-inl.h:90-96
  void initValues(const Trajectory& init_values) {
    if (!have_graph_) throw std::runtime_error("[ISAM2TrajOptimizer] initFactorGraph must come first");
    if (init_values.dof != dof_ || init_values.total_step != setting_.total_step)
      throw std::runtime_error("[ISAM2TrajOptimizer] init_values do not match dof / total_step");
    check(gpmp2mi_plan_set_problem(plan_, start_conf_.data(), start_vel_.data(), goal_conf_.data(), goal_vel_.data(),
                                   init_values.data.data()),
          "gpmp2mi_plan_set_problem");
    opt_values_ = init_values;
  }
  /// ISAM2TrajOptimizer-inl.h:102-114
  void update() {
    check(gpmp2mi_plan_update(plan_, 1, nullptr), "gpmp2mi_plan_update");
    int status = 0;
    check(gpmp2mi_plan_get_result(plan_, opt_values_.data.data(), nullptr, nullptr, &status, nullptr),
          "gpmp2mi_plan_get_result");
    if (status == GPMP2MI_TRAJ_NOT_SPD) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
  }
  /// ISAM2TrajOptimizer-inl.h:120-141
  void changeGoalConfigAndVel(const Vector& goal_conf, const Vector& goal_vel) {
    fits(goal_conf), fits(goal_vel);
    check(gpmp2mi_plan_change_goal(plan_, 0, goal_conf.data(), goal_vel.data()), "gpmp2mi_plan_change_goal");
  }
  /// ISAM2TrajOptimizer-inl.h:147-153
  void removeGoalConfigAndVel() { check(gpmp2mi_plan_remove_goal(plan_, 0), "gpmp2mi_plan_remove_goal"); }
  /// ISAM2TrajOptimizer-inl.h:159-168
  void fixConfigAndVel(std::size_t state_idx, const Vector& conf_fix, const Vector& vel_fix) {
    fits(conf_fix), fits(vel_fix);
    check(gpmp2mi_plan_fix_state(plan_, 0, static_cast<int>(state_idx), conf_fix.data(), vel_fix.data()),
          "gpmp2mi_plan_fix_state");
  }
  /// ISAM2TrajOptimizer-inl.h:174-180; pose_cov row-major [dof][dof]
  void addPoseEstimate(std::size_t state_idx, const Vector& pose, const Vector& pose_cov) {
    fits(pose);
    if (pose_cov.size() != dof_ * dof_) throw std::runtime_error("[ISAM2TrajOptimizer] covariance dim does not fit dof");
    check(gpmp2mi_plan_add_state_estimate(plan_, 0, static_cast<int>(state_idx), pose.data(), pose_cov.data(), nullptr,
                                          nullptr),
          "gpmp2mi_plan_add_state_estimate");
  }
  /// ISAM2TrajOptimizer-inl.h:186-195
  void addStateEstimate(std::size_t state_idx, const Vector& pose, const Vector& pose_cov, const Vector& vel,
                        const Vector& vel_cov) {
    fits(pose), fits(vel);
    if (pose_cov.size() != dof_ * dof_ || vel_cov.size() != dof_ * dof_)
      throw std::runtime_error("[ISAM2TrajOptimizer] covariance dim does not fit dof");
    check(gpmp2mi_plan_add_state_estimate(plan_, 0, static_cast<int>(state_idx), pose.data(), pose_cov.data(),
                                          vel.data(), vel_cov.data()),
          "gpmp2mi_plan_add_state_estimate");
  }
  const Trajectory& values() const { return opt_values_; }
  /// gtsam::ISAM2::marginalCovariance of (x_i, v_i) together: the 2 dof x 2 dof block of Sigma = H^-1 at the current
  /// estimate (gpmp2mi_plan_marginals), row-major, ordered [x_i; v_i]
  Vector jointMarginalCovariance(std::size_t state_idx) const {
    if (opt_values_.data.empty()) throw std::runtime_error("[ISAM2TrajOptimizer] initValues must come first");
    if (state_idx > setting_.total_step) throw std::runtime_error("[ISAM2TrajOptimizer] state_idx is past total_step");
    const std::size_t nn = 4 * dof_ * dof_;
    Vector all((setting_.total_step + 1) * nn);
    int ok = 0;
    check(gpmp2mi_plan_marginals(plan_, nullptr, all.data(), nullptr, &ok), "gpmp2mi_plan_marginals");
    if (!ok) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
    return Vector(all.begin() + state_idx * nn, all.begin() + (state_idx + 1) * nn);
  }
  /// gtsam::ISAM2::marginalCovariance(Symbol('x', i)) (velocity: Symbol('v', i)): row-major [dof][dof]
  Vector marginalCovariance(std::size_t state_idx, bool velocity = false) const {
    const Vector J = jointMarginalCovariance(state_idx);
    const std::size_t o = velocity ? dof_ : 0;
    Vector out(dof_ * dof_);
    for (std::size_t r = 0; r < dof_; r++)
      for (std::size_t c = 0; c < dof_; c++) out[r * dof_ + c] = J[(o + r) * 2 * dof_ + o + c];
    return out;
  }

 private:
  void fits(const Vector& v) const {
    if (v.size() != dof_) throw std::runtime_error("[ISAM2TrajOptimizer] vector dim does not fit dof");
  }
  std::size_t dof_;
  TrajOptimizerSetting setting_;
  gpmp2mi_plan* plan_ = nullptr;
  Vector start_conf_, start_vel_, goal_conf_, goal_vel_;
  Trajectory opt_values_;
  bool have_graph_ = false;
};
}  // namespace internal
/// gpmp2/planner/ISAM2TrajOptimizer.h:143-156
typedef internal::ISAM2TrajOptimizer<ArmModel, PlanarSDF> ISAM2TrajOptimizer2DArm;
typedef internal::ISAM2TrajOptimizer<ArmModel, SignedDistanceField> ISAM2TrajOptimizer3DArm;

/// The posterior around a result (include/gpmp2mi.h "posterior"): Sigma = H^-1 of the BatchTrajOptimize graph
/// linearized at `result`, what gtsam::Marginals(graph, result) holds.  diag [total_step+1][2 dof][2 dof] = the blocks
/// of (x_i, v_i), off [total_step][2 dof][2 dof] = block (i+1, i), both row-major.
struct TrajectoryCovariance {
  std::size_t dof = 0, total_step = 0;
  Vector diag, off;
  /// the [2 dof][2 dof] block of state i
  Vector joint(std::size_t i) const {
    const std::size_t nn = 4 * dof * dof;
    return Vector(diag.begin() + i * nn, diag.begin() + (i + 1) * nn);
  }
};
/// ROBOT: a robot model of at most 7 dof (one tile per block; wider ones throw); SDF: SignedDistanceField or PlanarSDF.
template <class ROBOT, class SDF>
inline TrajectoryCovariance TrajectoryMarginals(const ROBOT& robot, const SDF& sdf, const Trajectory& result,
                                                const Vector& start_conf, const Vector& start_vel, const Vector& end_conf,
                                                const Vector& end_vel, const TrajOptimizerSetting& setting) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[TrajectoryMarginals] result does not match dof / total_step");
  for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
    if (v->size() != robot.dof()) throw std::runtime_error("[TrajectoryMarginals] vector dim does not fit dof");
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, 1, &plan), "gpmp2mi_plan_create");
  TrajectoryCovariance out;
  out.dof = robot.dof(), out.total_step = setting.total_step;
  const std::size_t nn = 4 * out.dof * out.dof;
  out.diag.assign((out.total_step + 1) * nn, 0.0);
  out.off.assign(out.total_step * nn, 0.0);
  int ok = 0;
  int rc = gpmp2mi_plan_set_problem(plan, start_conf.data(), start_vel.data(), end_conf.data(), end_vel.data(),
                                    result.data.data());
  const char* what = "gpmp2mi_plan_set_problem";
  if (!rc) {
    rc = gpmp2mi_plan_marginals(plan, result.data.data(), out.diag.data(), out.off.data(), &ok);
    what = "gpmp2mi_plan_marginals";
  }
  gpmp2mi_plan_destroy(plan);
  check(rc, what);
  if (!ok) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
  return out;
}

/// The posterior on the executed timeline (include/gpmp2mi.h): how sure the planner is that the inter_step-up-sampled
/// `result` clears the obstacles.  robust_clearance = min over the in-range (checked state, sphere) pairs of
/// clearance - kappa sigma, sigma the first-order standard deviation of the clearance under TrajectoryMarginals' Sigma
/// carried to the checked states; worst_state / worst_sphere attain it (-1 if no pair is in range), sigma_worst is sigma
/// there; sigma [Md][nr_body_spheres], Md = total_step (inter_step + 1) + 1, NaN at pairs out of range.
/// The function below has the struct's name, as the entry point has: write `auto r = TrajectoryRisk(...)`.
struct TrajectoryRisk {
  std::size_t checked_states = 0, nr_spheres = 0;
  double robust_clearance = 0.0, sigma_worst = 0.0;
  int worst_state = -1, worst_sphere = -1, out_of_range = 0;
  Vector sigma;
  double sigma_at(std::size_t state, std::size_t sphere) const { return sigma[state * nr_spheres + sphere]; }
};
/// ROBOT: a vector-space robot model of at most 7 dof (wider ones and the Pose2 kinds throw); SDF: SignedDistanceField
/// or PlanarSDF.
template <class ROBOT, class SDF>
inline struct TrajectoryRisk TrajectoryRisk(const ROBOT& robot, const SDF& sdf, const Trajectory& result,
                                            const Vector& start_conf, const Vector& start_vel, const Vector& end_conf,
                                            const Vector& end_vel, const TrajOptimizerSetting& setting,
                                            std::size_t inter_step, double kappa) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[TrajectoryRisk] result does not match dof / total_step");
  for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
    if (v->size() != robot.dof()) throw std::runtime_error("[TrajectoryRisk] vector dim does not fit dof");
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, 1, &plan), "gpmp2mi_plan_create");
  struct TrajectoryRisk out;
  out.checked_states = setting.total_step * (inter_step + 1) + 1;
  out.nr_spheres = robot.nr_body_spheres();
  out.sigma.assign(out.checked_states * out.nr_spheres, 0.0);
  int ok = 0, worst[2] = {-1, -1};
  // the initial values of a plan that has not been optimized are its current estimate
  int rc = gpmp2mi_plan_set_problem(plan, start_conf.data(), start_vel.data(), end_conf.data(), end_vel.data(),
                                    result.data.data());
  const char* what = "gpmp2mi_plan_set_problem";
  if (!rc) {
    rc = gpmp2mi_plan_risk(plan, static_cast<int>(inter_step), kappa, &out.robust_clearance, worst, &out.sigma_worst,
                           &out.out_of_range, out.sigma.data(), &ok);
    what = "gpmp2mi_plan_risk";
  }
  gpmp2mi_plan_destroy(plan);
  check(rc, what);
  if (!ok) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
  out.worst_state = worst[0], out.worst_sphere = worst[1];
  return out;
}

/// The sampled clearance (include/gpmp2mi.h "sampled clearance"): K joint draws of the inter_step-up-sampled trajectory
/// from the posterior at `result`, each through the collision check.  hits = the samples whose minimum clearance lies
/// below required_clearance, probability = hits / K; clearance [K] and worst [K][2] per sample, state_hits [Md] per
/// checked state, Md = total_step (inter_step + 1) + 1; oor_samples = the samples with a pair out of range.
/// probability (or -hits) can be handed to SelectBest as a score by the caller.
/// The function below has the struct's name, as TrajectoryRisk: write `auto r = SampledClearance(...)`.
struct SampledClearance {
  std::size_t checked_states = 0, samples = 0;
  int hits = 0, oor_samples = 0;
  double probability = 0.0;
  Vector clearance;
  std::vector<int> worst, state_hits;
};
/// ROBOT, SDF as for TrajectoryRisk; inter_step <= 63.
template <class ROBOT, class SDF>
inline struct SampledClearance SampledClearance(const ROBOT& robot, const SDF& sdf, const Trajectory& result,
                                                const Vector& start_conf, const Vector& start_vel,
                                                const Vector& end_conf, const Vector& end_vel,
                                                const TrajOptimizerSetting& setting, std::size_t inter_step,
                                                std::size_t K, std::uint64_t seed, double required_clearance,
                                                bool bridge = true, int row_first = 0, int sample_first = 0) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[SampledClearance] result does not match dof / total_step");
  for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
    if (v->size() != robot.dof()) throw std::runtime_error("[SampledClearance] vector dim does not fit dof");
  if (K < 1) throw std::runtime_error("[SampledClearance] K must be >= 1");
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, 1, &plan), "gpmp2mi_plan_create");
  struct SampledClearance out;
  out.checked_states = setting.total_step * (inter_step + 1) + 1;
  out.samples = K;
  out.clearance.assign(K, 0.0);
  out.worst.assign(2 * K, -1);
  out.state_hits.assign(out.checked_states, 0);
  int ok = 0;
  // the initial values of a plan that has not been optimized are its current estimate
  int rc = gpmp2mi_plan_set_problem(plan, start_conf.data(), start_vel.data(), end_conf.data(), end_vel.data(),
                                    result.data.data());
  const char* what = "gpmp2mi_plan_set_problem";
  if (!rc) {
    rc = gpmp2mi_plan_collision_probability(plan, static_cast<int>(inter_step), static_cast<int>(K), seed, row_first,
                                            sample_first, bridge ? 1 : 0, required_clearance, &out.hits,
                                            &out.probability, out.clearance.data(), out.worst.data(), nullptr,
                                            out.state_hits.data(), &out.oor_samples, &ok);
    what = "gpmp2mi_plan_collision_probability";
  }
  gpmp2mi_plan_destroy(plan);
  check(rc, what);
  if (!ok) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
  return out;
}

/// Seeding on the device (include/gpmp2mi.h "seeding").  Not in the reference, where restarts are the caller's business.
/// out [a_count][b_count][nblk][n] of the library's counter RNG: normal(seed, stream, a_first + a, b_first + b, i, r)
inline Vector NormalFill(std::uint64_t seed, int stream, int a_first, int a_count, int b_first, int b_count, int nblk, int n) {
  Vector out(static_cast<std::size_t>(a_count) * b_count * nblk * n);
  check(gpmp2mi_normal_fill(seed, stream, a_first, a_count, b_first, b_count, nblk, n, out.data()), "gpmp2mi_normal_fill");
  return out;
}
/// M restarts from start_conf to end_conf and what the optimizer made of them: restart j = first + row starts from the
/// straight line plus scale * (a draw from the plan's GP-prior bridge, a function of (seed, j) alone); keep_first:
/// restart 0 is the straight line itself.  `init` is filled by SeedRestarts and, on request, by BatchTrajOptimizeSeeded.
struct SeededRestarts {
  std::vector<Trajectory> init, traj;
  std::vector<int> iterations, status;
  Vector final_error;
};
namespace internal {
inline std::vector<Trajectory> split_rows(const Vector& flat, std::size_t M, std::size_t dof, std::size_t total_step) {
  const std::size_t T = (total_step + 1) * 2 * dof;
  std::vector<Trajectory> out(M, Trajectory(dof, total_step));
  for (std::size_t m = 0; m < M; m++) std::copy(flat.begin() + m * T, flat.begin() + (m + 1) * T, out[m].data.begin());
  return out;
}
inline Vector repeat_rows(const Vector& v, std::size_t M) {
  Vector out(M * v.size());
  for (std::size_t m = 0; m < M; m++) std::copy(v.begin(), v.end(), out.begin() + m * v.size());
  return out;
}
}  // namespace internal
/// ROBOT: a vector-space robot model of at most 7 dof (others throw); SDF: SignedDistanceField or PlanarSDF.
template <class ROBOT, class SDF>
inline std::vector<Trajectory> SeedRestarts(const ROBOT& robot, const SDF& sdf, const Vector& start_conf,
                                            const Vector& end_conf, const TrajOptimizerSetting& setting, std::size_t M,
                                            std::uint64_t seed, double scale = 1.0, bool keep_first = true, int first = 0) {
  if (start_conf.size() != robot.dof() || end_conf.size() != robot.dof())
    throw std::runtime_error("[SeedRestarts] vector dim does not fit dof");
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, 1, &plan), "gpmp2mi_plan_create");
  const Vector sc = internal::repeat_rows(start_conf, M), ec = internal::repeat_rows(end_conf, M);
  Vector init(M * (setting.total_step + 1) * 2 * robot.dof());
  const int rc = gpmp2mi_plan_seed_restarts(plan, static_cast<int>(M), seed, first, scale, keep_first ? 1 : 0, sc.data(),
                                            ec.data(), nullptr, init.data());
  gpmp2mi_plan_destroy(plan);
  check(rc, "gpmp2mi_plan_seed_restarts");
  return internal::split_rows(init, M, robot.dof(), setting.total_step);
}
/// The M restarts through a plan of `slots` slots (gpmp2mi_plan_optimize_queue_seeded): no trajectory crosses to the
/// device.  The rows equal SeedRestarts followed by one BatchTrajOptimize per row.
template <class ROBOT, class SDF>
inline SeededRestarts BatchTrajOptimizeSeeded(const ROBOT& robot, const SDF& sdf, const Vector& start_conf,
                                              const Vector& start_vel, const Vector& end_conf, const Vector& end_vel,
                                              const TrajOptimizerSetting& setting, std::size_t M, std::size_t slots,
                                              std::uint64_t seed, double scale = 1.0, bool keep_first = true,
                                              bool want_init = false, int first = 0) {
  for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
    if (v->size() != robot.dof()) throw std::runtime_error("[BatchTrajOptimizeSeeded] vector dim does not fit dof");
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, static_cast<int>(slots), &plan), "gpmp2mi_plan_create");
  const Vector sc = internal::repeat_rows(start_conf, M), sv = internal::repeat_rows(start_vel, M),
               ec = internal::repeat_rows(end_conf, M), ev = internal::repeat_rows(end_vel, M);
  const std::size_t T = (setting.total_step + 1) * 2 * robot.dof();
  Vector traj(M * T), init(want_init ? M * T : 0);
  SeededRestarts out;
  out.iterations.assign(M, 0);
  out.status.assign(M, 0);
  out.final_error.assign(M, 0.0);
  const int rc = gpmp2mi_plan_optimize_queue_seeded(plan, static_cast<int>(M), seed, first, scale, keep_first ? 1 : 0,
                                                    sc.data(), sv.data(), ec.data(), ev.data(), nullptr, traj.data(),
                                                    out.iterations.data(), out.final_error.data(), out.status.data(),
                                                    nullptr, want_init ? init.data() : nullptr);
  gpmp2mi_plan_destroy(plan);
  check(rc, "gpmp2mi_plan_optimize_queue_seeded");
  out.traj = internal::split_rows(traj, M, robot.dof(), setting.total_step);
  if (want_init) out.init = internal::split_rows(init, M, robot.dof(), setting.total_step);
  return out;
}
/// K perturbations delta ~ N(0, Sigma) of `result` (TrajectoryMarginals' Sigma), drawn on the device: sample s is a
/// function of (seed, sample_first + s) alone.  result + delta is a trajectory drawn from the posterior.
template <class ROBOT, class SDF>
inline std::vector<Trajectory> TrajectoryPosteriorSamples(const ROBOT& robot, const SDF& sdf, const Trajectory& result,
                                                          const Vector& start_conf, const Vector& start_vel,
                                                          const Vector& end_conf, const Vector& end_vel,
                                                          const TrajOptimizerSetting& setting, std::size_t K,
                                                          std::uint64_t seed, int sample_first = 0) {
  if (result.dof != robot.dof() || result.total_step != setting.total_step)
    throw std::runtime_error("[TrajectoryPosteriorSamples] result does not match dof / total_step");
  for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
    if (v->size() != robot.dof()) throw std::runtime_error("[TrajectoryPosteriorSamples] vector dim does not fit dof");
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, 1, &plan), "gpmp2mi_plan_create");
  Vector delta(K * result.data.size());
  int ok = 0;
  int rc = gpmp2mi_plan_set_problem(plan, start_conf.data(), start_vel.data(), end_conf.data(), end_vel.data(),
                                    result.data.data());
  const char* what = "gpmp2mi_plan_set_problem";
  if (!rc) {
    rc = gpmp2mi_plan_sample_posterior_seeded(plan, static_cast<int>(K), seed, 0, sample_first, delta.data(), &ok);
    what = "gpmp2mi_plan_sample_posterior_seeded";
  }
  gpmp2mi_plan_destroy(plan);
  check(rc, what);
  if (!ok) throw std::runtime_error("[gpmp2mi] IndeterminantLinearSystemException");
  return internal::split_rows(delta, K, robot.dof(), setting.total_step);
}

/// The modes among several results (include/gpmp2mi.h "distinct alternatives"): mode[b] is the mode of result b in leader
/// order (-1: the row does not take part), leaders[k] the best-ranked row of mode k, sizes[k] its member count.
struct TrajectoryGroups {
  std::vector<int> mode, leaders, sizes;   // leaders / sizes hold n_modes entries
  std::size_t n_modes = 0;
};
namespace internal {
inline void trim_groups(TrajectoryGroups& g, int n_modes) {
  g.n_modes = static_cast<std::size_t>(n_modes);
  g.leaders.resize(g.n_modes);
  g.sizes.resize(g.n_modes);
}
}  // namespace internal
/// The leader rule on a given symmetric distance matrix dist [B][B] row-major: results are visited by ascending score
/// (the lowest index on ties) and join the first leader within `radius`, or become the next leader.  eligible may be
/// empty (all take part); a non-finite score does not take part.  Host code.
inline TrajectoryGroups GroupRows(const Vector& dist, const Vector& score, const std::vector<int>& eligible, double radius) {
  const std::size_t B = score.size();
  if (dist.size() != B * B || (!eligible.empty() && eligible.size() != B))
    throw std::runtime_error("[GroupRows] dist, score and eligible differ in size");
  TrajectoryGroups g;
  g.mode.assign(B, -1);
  g.leaders.assign(B, -1);
  g.sizes.assign(B, 0);
  int n = 0;
  check(gpmp2mi_group_rows(static_cast<int>(B), dist.data(), score.data(), eligible.empty() ? nullptr : eligible.data(),
                           radius, g.mode.data(), g.leaders.data(), g.sizes.data(), &n),
        "gpmp2mi_group_rows");
  internal::trim_groups(g, n);
  return g;
}
/// The same from the trajectories themselves, distances and rule on the device: metric GPMP2MI_DIST_MAX_STATE (the
/// largest weighted configuration distance over the support states) or GPMP2MI_DIST_RMS; weights may be empty (all 1).
inline TrajectoryGroups GroupTrajectories(const std::vector<Trajectory>& results, const Vector& score,
                                          const std::vector<int>& eligible, double radius,
                                          int metric = GPMP2MI_DIST_MAX_STATE, const Vector& weights = {}) {
  const std::size_t B = results.size();
  if (B == 0 || score.size() != B || (!eligible.empty() && eligible.size() != B))
    throw std::runtime_error("[GroupTrajectories] results, score and eligible differ in length");
  const std::size_t dof = results[0].dof, N = results[0].total_step;
  if (!weights.empty() && weights.size() != dof) throw std::runtime_error("[GroupTrajectories] weights dim does not fit dof");
  Vector flat;
  for (const Trajectory& t : results) {
    if (t.dof != dof || t.total_step != N) throw std::runtime_error("[GroupTrajectories] results differ in shape");
    flat.insert(flat.end(), t.data.begin(), t.data.end());
  }
  TrajectoryGroups g;
  g.mode.assign(B, -1);
  g.leaders.assign(B, -1);
  g.sizes.assign(B, 0);
  int n = 0;
  check(gpmp2mi_group_traj(static_cast<int>(dof), static_cast<int>(B), static_cast<int>(N), flat.data(),
                           weights.empty() ? nullptr : weights.data(), metric, radius, score.data(),
                           eligible.empty() ? nullptr : eligible.data(), g.mode.data(), g.leaders.data(), g.sizes.data(), &n),
        "gpmp2mi_group_traj");
  internal::trim_groups(g, n);
  return g;
}
/// One representative per mode of a batch of restarts, best first (gpmp2mi_plan_select_distinct): alt[k] is the restart
/// leading mode k, alt_size[k] its member count, alt_error[k] its final error, traj[k] / dense[k] its trajectory and the
/// inter_step-up-sampled form; n_modes counts all modes, the vectors hold min(n_modes, max_alt) entries.
struct DistinctAlternatives {
  std::size_t n_modes = 0, n_eligible = 0;
  std::vector<int> alt, alt_size, mode;
  Vector alt_error;
  std::vector<Trajectory> traj, dense;
};
/// BatchTrajOptimize from every row of init_values, then the dense collision check, the selection rule of
/// SelectBestTrajectory and the grouping of the eligible results, all on the device; alt[0] is the result
/// SelectBestTrajectory picks.  pairs (may be null) adds the self-collision rule.
template <class ROBOT, class SDF>
inline DistinctAlternatives BatchTrajOptimizeDistinct(const ROBOT& robot, const SDF& sdf, const Vector& start_conf,
                                                      const Vector& start_vel, const Vector& end_conf, const Vector& end_vel,
                                                      const std::vector<Trajectory>& init_values,
                                                      const TrajOptimizerSetting& setting, std::size_t inter_step,
                                                      double radius, std::size_t max_alt = 8, double required_clearance = 0.0,
                                                      bool require_in_range = false, int metric = GPMP2MI_DIST_MAX_STATE,
                                                      const Vector& weights = {}, const SelfCollisionPairs* pairs = nullptr,
                                                      double required_self_clearance = 0.0) {
  const std::size_t B = init_values.size(), dof = robot.dof(), N = setting.total_step;
  for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
    if (v->size() != dof) throw std::runtime_error("[BatchTrajOptimizeDistinct] vector dim does not fit dof");
  if (B == 0 || (!weights.empty() && weights.size() != dof))
    throw std::runtime_error("[BatchTrajOptimizeDistinct] no initial values, or weights dim does not fit dof");
  if (max_alt < 1 || max_alt > GPMP2MI_MAX_ALTERNATIVES)
    throw std::runtime_error("[BatchTrajOptimizeDistinct] max_alt must be in 1..GPMP2MI_MAX_ALTERNATIVES");
  Vector init;
  for (const Trajectory& t : init_values) {
    if (t.dof != dof || t.total_step != N) throw std::runtime_error("[BatchTrajOptimizeDistinct] init does not match dof / total_step");
    init.insert(init.end(), t.data.begin(), t.data.end());
  }
  const gpmp2mi_settings s = setting.c_struct();
  gpmp2mi_plan* plan = nullptr;
  check(gpmp2mi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, static_cast<int>(B), &plan), "gpmp2mi_plan_create");
  const Vector sc = internal::repeat_rows(start_conf, B), sv = internal::repeat_rows(start_vel, B),
               ec = internal::repeat_rows(end_conf, B), ev = internal::repeat_rows(end_vel, B);
  const std::size_t Md = N * (inter_step + 1) + 1;
  DistinctAlternatives out;
  out.alt.assign(max_alt, -1);
  out.alt_size.assign(max_alt, 0);
  out.alt_error.assign(max_alt, 0.0);
  out.mode.assign(B, -1);
  Vector ta(max_alt * (N + 1) * 2 * dof), da(max_alt * Md * 2 * dof);
  int nm = 0, ne = 0;
  int rc = gpmp2mi_plan_set_problem(plan, sc.data(), sv.data(), ec.data(), ev.data(), init.data());
  const char* what = "gpmp2mi_plan_set_problem";
  if (!rc) {
    rc = gpmp2mi_plan_optimize(plan, nullptr);
    what = "gpmp2mi_plan_optimize";
  }
  if (!rc) {
    rc = gpmp2mi_plan_select_distinct(plan, static_cast<int>(inter_step), required_clearance, require_in_range ? 1 : 0,
                                      pairs ? pairs->handle() : nullptr, required_self_clearance, metric,
                                      weights.empty() ? nullptr : weights.data(), radius, static_cast<int>(max_alt), &nm, &ne,
                                      out.alt.data(), out.alt_size.data(), out.alt_error.data(), out.mode.data(), ta.data(),
                                      da.data());
    what = "gpmp2mi_plan_select_distinct";
  }
  gpmp2mi_plan_destroy(plan);
  check(rc, what);
  out.n_modes = static_cast<std::size_t>(nm);
  out.n_eligible = static_cast<std::size_t>(ne);
  const std::size_t k = std::min(out.n_modes, max_alt);
  out.alt.resize(k);
  out.alt_size.resize(k);
  out.alt_error.resize(k);
  ta.resize(k * (N + 1) * 2 * dof);
  da.resize(k * Md * 2 * dof);
  out.traj = internal::split_rows(ta, k, dof, N);
  out.dense = internal::split_rows(da, k, dof, Md - 1);
  return out;
}

/// B independent BatchTrajOptimize problems of one robot, field and setting, sharded over several GPUs of this process
/// (gpmp2mi_multi_plan, include/gpmp2mi.h): shard k of `devices` holds a contiguous share of the rows, repeats allowed.
/// The robot model and the field must outlive the planner.  Not in the reference (one problem per call there).
class MultiDeviceBatchPlanner {
 public:
  template <class ROBOT, class SDF>
  MultiDeviceBatchPlanner(const ROBOT& robot, const SDF& sdf, const TrajOptimizerSetting& setting, std::size_t B,
                          const std::vector<int>& devices)
      : dof_(robot.dof()), setting_(setting), B_(B) {
    if (devices.empty()) throw std::runtime_error("[MultiDeviceBatchPlanner] devices must name at least one device");
    const gpmp2mi_settings s = setting_.c_struct();
    check(gpmp2mi_multi_plan_create(robot.handle(), sdf.handle(), &s, nullptr, static_cast<int>(B),
                                    static_cast<int>(devices.size()), devices.data(), &plan_),
          "gpmp2mi_multi_plan_create");
  }
  ~MultiDeviceBatchPlanner() {
    if (plan_) gpmp2mi_multi_plan_destroy(plan_);
  }
  MultiDeviceBatchPlanner(const MultiDeviceBatchPlanner&) = delete;
  MultiDeviceBatchPlanner& operator=(const MultiDeviceBatchPlanner&) = delete;

  /// B problems, one entry per problem; returns the optimized trajectories in the same order
  std::vector<Trajectory> optimize(const std::vector<Vector>& start_conf, const std::vector<Vector>& start_vel,
                                   const std::vector<Vector>& end_conf, const std::vector<Vector>& end_vel,
                                   const std::vector<Trajectory>& init_values) {
    const std::size_t D = dof_, T = (setting_.total_step + 1) * 2 * D;
    Vector sc(B_ * D), sv(B_ * D), ec(B_ * D), ev(B_ * D), init(B_ * T);
    auto rows = [&](const std::vector<Vector>& in, Vector& out, const char* name) {
      if (in.size() != B_) throw std::runtime_error(std::string("[MultiDeviceBatchPlanner] ") + name + ": expected B entries");
      for (std::size_t b = 0; b < B_; b++) {
        if (in[b].size() != D) throw std::runtime_error(std::string("[MultiDeviceBatchPlanner] ") + name + " dim does not fit dof");
        std::copy(in[b].begin(), in[b].end(), out.begin() + b * D);
      }
    };
    rows(start_conf, sc, "start_conf");
    rows(start_vel, sv, "start_vel");
    rows(end_conf, ec, "end_conf");
    rows(end_vel, ev, "end_vel");
    if (init_values.size() != B_) throw std::runtime_error("[MultiDeviceBatchPlanner] init_values: expected B entries");
    for (std::size_t b = 0; b < B_; b++) {
      if (init_values[b].dof != D || init_values[b].total_step != setting_.total_step)
        throw std::runtime_error("[MultiDeviceBatchPlanner] init_values do not match dof / total_step");
      std::copy(init_values[b].data.begin(), init_values[b].data.end(), init.begin() + b * T);
    }
    check(gpmp2mi_multi_plan_set_problem(plan_, sc.data(), sv.data(), ec.data(), ev.data(), init.data()),
          "gpmp2mi_multi_plan_set_problem");
    check(gpmp2mi_multi_plan_optimize(plan_), "gpmp2mi_multi_plan_optimize");
    Vector traj(B_ * T);
    iters_.assign(B_, 0);
    status_.assign(B_, 0);
    check(gpmp2mi_multi_plan_get_result(plan_, traj.data(), iters_.data(), nullptr, status_.data(), nullptr),
          "gpmp2mi_multi_plan_get_result");
    std::vector<Trajectory> out(B_, Trajectory(D, setting_.total_step));
    for (std::size_t b = 0; b < B_; b++) std::copy(traj.begin() + b * T, traj.begin() + (b + 1) * T, out[b].data.begin());
    return out;
  }
  /// BatchTrajOptimizeSeeded over the shards (gpmp2mi_multi_plan_optimize_queue_seeded): M restarts of one problem, the
  /// rows those of one plan
  SeededRestarts optimizeSeeded(const Vector& start_conf, const Vector& start_vel, const Vector& end_conf,
                                const Vector& end_vel, std::size_t M, std::uint64_t seed, double scale = 1.0,
                                bool keep_first = true, int first = 0) {
    for (const Vector* v : {&start_conf, &start_vel, &end_conf, &end_vel})
      if (v->size() != dof_) throw std::runtime_error("[MultiDeviceBatchPlanner] vector dim does not fit dof");
    const Vector sc = internal::repeat_rows(start_conf, M), sv = internal::repeat_rows(start_vel, M),
                 ec = internal::repeat_rows(end_conf, M), ev = internal::repeat_rows(end_vel, M);
    Vector traj(M * (setting_.total_step + 1) * 2 * dof_);
    SeededRestarts out;
    out.iterations.assign(M, 0);
    out.status.assign(M, 0);
    out.final_error.assign(M, 0.0);
    check(gpmp2mi_multi_plan_optimize_queue_seeded(plan_, static_cast<int>(M), seed, first, scale, keep_first ? 1 : 0,
                                                   sc.data(), sv.data(), ec.data(), ev.data(), nullptr, traj.data(),
                                                   out.iterations.data(), out.final_error.data(), out.status.data(),
                                                   nullptr, nullptr),
          "gpmp2mi_multi_plan_optimize_queue_seeded");
    out.traj = internal::split_rows(traj, M, dof_, setting_.total_step);
    return out;
  }
  /// of the last optimize, per problem: GTSAM iterations() and GPMP2MI_TRAJ_* status
  const std::vector<int>& iterations() const { return iters_; }
  const std::vector<int>& status() const { return status_; }
  /// shard k holds problems row_begin()[k] .. row_begin()[k + 1] - 1 on devices()[k]
  std::vector<int> devices() const { return shards().first; }
  std::vector<int> row_begin() const { return shards().second; }

 private:
  std::pair<std::vector<int>, std::vector<int>> shards() const {
    int n = 0;
    check(gpmp2mi_multi_plan_shards(plan_, &n, nullptr, nullptr), "gpmp2mi_multi_plan_shards");
    std::vector<int> dev(n), rb(n + 1);
    check(gpmp2mi_multi_plan_shards(plan_, &n, dev.data(), rb.data()), "gpmp2mi_multi_plan_shards");
    return {dev, rb};
  }
  std::size_t dof_;
  TrajOptimizerSetting setting_;
  std::size_t B_;
  gpmp2mi_multi_plan* plan_ = nullptr;
  std::vector<int> iters_, status_;
};

#ifdef GPMP2MI_HAVE_GTSAM
/// gtsam::Values (keys Symbol('x', i) / Symbol('v', i), gpmp2/planner/BatchTrajOptimizer.h:39-41) <-> Trajectory
inline Trajectory fromValues(const gtsam::Values& values, std::size_t dof, std::size_t total_step) {
  Trajectory t(dof, total_step);
  for (std::size_t i = 0; i <= total_step; i++) {
    const gtsam::Vector x = values.at<gtsam::Vector>(gtsam::Symbol('x', i));
    const gtsam::Vector v = values.at<gtsam::Vector>(gtsam::Symbol('v', i));
    for (std::size_t k = 0; k < dof; k++) {
      t.x(i)[k] = x(k);
      t.v(i)[k] = v(k);
    }
  }
  return t;
}
inline gtsam::Values toValues(const Trajectory& t) {
  gtsam::Values values;
  for (std::size_t i = 0; i <= t.total_step; i++) {
    gtsam::Vector x(t.dof), v(t.dof);
    for (std::size_t k = 0; k < t.dof; k++) {
      x(k) = t.x(i)[k];
      v(k) = t.v(i)[k];
    }
    values.insert(gtsam::Symbol('x', i), x);
    values.insert(gtsam::Symbol('v', i), v);
  }
  return values;
}
#endif

}  // namespace gpmp2mi
