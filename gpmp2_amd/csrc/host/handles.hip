// handles.hip -- last error, version, device count; robot and field handles; default settings; the host-side GP
// constants (the eight Lambda / Psi scalars per sub-step, W^-1) the factor calls and plan creation share.
#include <cmath>
#include <cstring>
#include <fstream>
#include <numeric>

#include "host.h"

namespace g2 {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
const std::string& last_error() { return g_last_error; }

int ensure_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error("no usable HIP device (this library has no CPU fallback)");
    return GPMP2MI_ERR_NO_DEVICE;
  }
  return GPMP2MI_OK;
}

// 2x2 scalar GP matrices (gpmp2/gp/GPutils.h:25-59 with Qc factored out)
static void mm2(const double A[4], const double B[4], double C[4]) {
  const double c0 = A[0] * B[0] + A[1] * B[2], c1 = A[0] * B[1] + A[1] * B[3];
  const double c2 = A[2] * B[0] + A[3] * B[2], c3 = A[2] * B[1] + A[3] * B[3];
  C[0] = c0; C[1] = c1; C[2] = c2; C[3] = c3;
}
void gp_winv(double dt, double W[4]) {
  W[0] = 12.0 * std::pow(dt, -3.0);
  W[1] = W[2] = (-6.0) * std::pow(dt, -2.0);
  W[3] = 4.0 * std::pow(dt, -1.0);
}
GpCoef gp_coef(double dt, double tau) {
  const double A[4] = {1.0 / 3 * std::pow(tau, 3.0), 1.0 / 2 * std::pow(tau, 2.0),
                       1.0 / 2 * std::pow(tau, 2.0), tau};
  const double CtT[4] = {1.0, 0.0, dt - tau, 1.0};  // Phi(dt - tau)^T
  double W[4], T[4], Psi[4], PC[4];
  gp_winv(dt, W);
  mm2(A, CtT, T);
  mm2(T, W, Psi);
  const double Cdt[4] = {1.0, dt, 0.0, 1.0};
  mm2(Psi, Cdt, PC);
  return GpCoef{1.0 - PC[0], tau - PC[1], 0.0 - PC[2], 1.0 - PC[3], Psi[0], Psi[1], Psi[2], Psi[3]};   // Lambda, Psi
}

bool invert_small(int n, const double* A, double* Ainv) {
  std::vector<double> M(A, A + n * n);
  for (int i = 0; i < n * n; i++) Ainv[i] = 0.0;
  for (int i = 0; i < n; i++) Ainv[i * n + i] = 1.0;
  for (int c = 0; c < n; c++) {
    int p = c;
    for (int i = c + 1; i < n; i++)
      if (std::fabs(M[i * n + c]) > std::fabs(M[p * n + c])) p = i;
    if (M[p * n + c] == 0.0) return false;
    if (p != c)
      for (int j = 0; j < n; j++) {
        std::swap(M[p * n + j], M[c * n + j]);
        std::swap(Ainv[p * n + j], Ainv[c * n + j]);
      }
    const double inv = 1.0 / M[c * n + c];
    for (int j = 0; j < n; j++) {
      M[c * n + j] *= inv;
      Ainv[c * n + j] *= inv;
    }
    for (int i = 0; i < n; i++) {
      if (i == c) continue;
      const double f = M[i * n + c];
      if (f == 0.0) continue;
      for (int j = 0; j < n; j++) {
        M[i * n + j] -= f * M[c * n + j];
        Ainv[i * n + j] -= f * Ainv[c * n + j];
      }
    }
  }
  return true;
}

std::atomic<long> g_robot_replicas{0}, g_sdf_replicas{0};

int sdf_alloc(int dim, const double origin[3], double cell, int nx, int ny, int nz, std::unique_ptr<gpmp2mi_sdf>& s) {
  G2_CHECK(dim == 2 || dim == 3, GPMP2MI_ERR_INVALID, "dim must be 2 or 3");
  G2_CHECK(nx > 0 && ny > 0 && nz > 0 && cell > 0, GPMP2MI_ERR_INVALID, "bad field size");
  G2_TRY(ensure_device());
  s = std::make_unique<gpmp2mi_sdf>();
  G2_HIP(hipGetDevice(&s->device));
  const size_t n = (size_t)nx * ny * nz;
  SdfDev& h = s->h;
  h.dim = dim;
  h.nx = nx;
  h.ny = ny;
  h.nz = nz;
  h.ox = origin[0];
  h.oy = origin[1];
  h.oz = dim == 3 ? origin[2] : 0.0;
  h.cell = cell;
  h.inv_cell = 1.0 / cell;
  // upper faces exactly as SignedDistanceField.h:105-107: origin + (n - 1.0) * cell_size
  h.hix = h.ox + (nx - 1.0) * cell;
  h.hiy = h.oy + (ny - 1.0) * cell;
  h.hiz = h.oz + (nz - 1.0) * cell;
  G2_HIP(hipMalloc((void**)&s->plain, n * sizeof(double)));
  const int nc = dim == 3 ? 8 : 4;
  G2_HIP(hipMalloc((void**)&s->cells, n * nc * sizeof(double)));
  h.plain = s->plain;
  h.cells = s->cells;
  return GPMP2MI_OK;
}

// caller layout -> [nz][ny][nx]
const double* to_zyx(const double* vox, int layout, int nx, int ny, int nz, std::vector<double>& tmp) {
  if (layout != GPMP2MI_SDF_LAYOUT_GTSAM) return vox;
  tmp.resize((size_t)nx * ny * nz);
  for (int z = 0; z < nz; z++)
    for (int y = 0; y < ny; y++)
      for (int x = 0; x < nx; x++) tmp[((size_t)z * ny + y) * nx + x] = vox[((size_t)z * nx + x) * ny + y];
  return tmp.data();
}
}  // namespace g2

using namespace g2;

extern "C" {

const char* gpmp2mi_last_error(void) { return last_error().c_str(); }
int gpmp2mi_version(void) { return GPMP2MI_VERSION; }
int gpmp2mi_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// -------------------------------------------------------------------------------------------- robot
int gpmp2mi_robot_create(const gpmp2mi_robot_desc* d, gpmp2mi_robot** out) {
  G2_CHECK(d && out, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  G2_CHECK(d->kind >= 0 && d->kind <= GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_2ARMS, GPMP2MI_ERR_INVALID, "unknown robot kind");
  G2_CHECK(d->arm_dof >= 0 && d->arm_dof <= MAXJ, GPMP2MI_ERR_UNSUPPORTED, "more than 14 arm joints");
  G2_CHECK(d->nr_spheres >= 0 && d->nr_spheres <= MAXS, GPMP2MI_ERR_UNSUPPORTED, "too many body spheres");
  const bool mobile = d->kind >= GPMP2MI_ROBOT_POSE2_MOBILE_BASE;
  const bool lift = d->kind == GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_ARM || d->kind == GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_2ARMS;
  const bool two = d->kind == GPMP2MI_ROBOT_POSE2_MOBILE_2ARMS || d->kind == GPMP2MI_ROBOT_POSE2_MOBILE_VETLIN_2ARMS;
  const int base = mobile ? 3 : 0;
  const int dof = (d->kind == GPMP2MI_ROBOT_POINT) ? 2 : base + (lift ? 1 : 0) + d->arm_dof;
  G2_CHECK(d->dof == dof, GPMP2MI_ERR_INVALID, "dof does not match robot kind / arm_dof");
  G2_CHECK(dof <= MAXD, GPMP2MI_ERR_UNSUPPORTED, "total dof > 18");
  if (d->kind == GPMP2MI_ROBOT_ARM || d->kind >= GPMP2MI_ROBOT_POSE2_MOBILE_ARM)
    G2_CHECK(d->arm_dof > 0 && d->a && d->alpha && d->d, GPMP2MI_ERR_INVALID, "missing DH parameters");
  if (two) G2_CHECK(d->arm2_dof > 0 && d->arm2_dof < d->arm_dof, GPMP2MI_ERR_INVALID, "arm2_dof must split arm_dof into two arms");
  G2_TRY(ensure_device());
  auto r = std::make_unique<gpmp2mi_robot>();
  RobotDev& h = r->h;
  std::memset(&h, 0, sizeof(h));
  h.kind = d->kind;
  h.dof = dof;
  h.arm_dof = d->arm_dof;
  h.arm2_dof = two ? d->arm2_dof : 0;
  h.reverse_linact = lift ? (d->reverse_linact != 0) : 0;
  h.base_dof = base;
  h.nr_links = (d->kind == GPMP2MI_ROBOT_ARM) ? d->arm_dof : mobile ? 1 + (lift ? 1 : 0) + d->arm_dof : 1;
  h.nr_spheres = d->nr_spheres;
  for (int j = 0; j < d->arm_dof; j++) {
    h.a[j] = d->a[j];
    h.d[j] = d->d[j];
    h.ca[j] = std::cos(d->alpha[j]);
    h.sa[j] = std::sin(d->alpha[j]);
    h.bias[j] = d->theta_bias ? d->theta_bias[j] : 0.0;
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) {
      h.base[i * 4 + j] = d->base_pose[i * 4 + j];
      h.base2[i * 4 + j] = (lift || two) ? d->base_pose2[i * 4 + j] : (i == j ? 1.0 : 0.0);
      h.base3[i * 4 + j] = (lift && two) ? d->base_pose3[i * 4 + j] : (i == j ? 1.0 : 0.0);
    }
  // sort spheres by link (stable) so the kinematic chain visits them in order
  std::vector<int> order(d->nr_spheres);
  std::iota(order.begin(), order.end(), 0);
  for (int s = 0; s < d->nr_spheres; s++)
    G2_CHECK(d->sphere_link[s] >= 0 && d->sphere_link[s] < h.nr_links, GPMP2MI_ERR_INVALID,
             "sphere link id out of range");
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return d->sphere_link[a] < d->sphere_link[b]; });
  for (int s = 0; s < d->nr_spheres; s++) {
    const int o = order[s];
    h.sph_link[s] = d->sphere_link[o];
    h.sph_orig[s] = o;
    h.sph_r[s] = d->sphere_radius[o];
    for (int i = 0; i < 3; i++) h.sph_c[3 * s + i] = d->sphere_center[3 * o + i];
  }
  int s = 0;
  for (int l = 0; l <= h.nr_links; l++) {
    while (s < d->nr_spheres && h.sph_link[s] < l) s++;
    h.link_first[l] = s;
  }
  h.link_first[h.nr_links] = d->nr_spheres;
  G2_HIP(hipGetDevice(&r->device));
  G2_HIP(hipMalloc((void**)&r->d, sizeof(RobotDev)));
  G2_HIP(hipMemcpy(r->d, &h, sizeof(RobotDev), hipMemcpyHostToDevice));
  *out = r.release();
  return GPMP2MI_OK;
}
void gpmp2mi_robot_destroy(gpmp2mi_robot* r) { delete r; }
int gpmp2mi_robot_dof(const gpmp2mi_robot* r) { return r ? r->h.dof : -1; }
int gpmp2mi_robot_nr_links(const gpmp2mi_robot* r) { return r ? r->h.nr_links : -1; }
int gpmp2mi_robot_nr_spheres(const gpmp2mi_robot* r) { return r ? r->h.nr_spheres : -1; }

int gpmp2mi_sdf_create(int dim, const double origin[3], double cell, int nx, int ny, int nz,
                       const double* vox, int layout, gpmp2mi_sdf** out) {
  G2_CHECK(out && origin && vox, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  if (dim == 2) nz = 1;
  G2_CHECK(layout == GPMP2MI_SDF_LAYOUT_ZYX || layout == GPMP2MI_SDF_LAYOUT_GTSAM, GPMP2MI_ERR_INVALID,
           "unknown voxel layout");
  std::unique_ptr<gpmp2mi_sdf> s;
  G2_TRY(sdf_alloc(dim, origin, cell, nx, ny, nz, s));
  std::vector<double> tmp;
  const double* src = to_zyx(vox, layout, nx, ny, nz, tmp);
  G2_HIP(hipMemcpy(s->plain, src, (size_t)nx * ny * nz * sizeof(double), hipMemcpyHostToDevice));
  G2_TRY(launch_sdf_pack(s->h, s->cells, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  *out = s.release();
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_field_from_occupancy(int dim, int nx, int ny, int nz, const double* occ, double cell,
                                     double* field) {
  G2_CHECK(occ && field, GPMP2MI_ERR_INVALID, "null argument");
  G2_CHECK(dim == 2 || dim == 3, GPMP2MI_ERR_INVALID, "dim must be 2 or 3");
  if (dim == 2) nz = 1;
  G2_CHECK(nx > 0 && ny > 0 && nz > 0 && cell > 0, GPMP2MI_ERR_INVALID, "bad grid size");
  G2_TRY(ensure_device());
  const size_t n = (size_t)nx * ny * nz;
  DevBuf<double> d_occ, d_field;
  DevBuf<int> wa, wb;
  G2_TRY(d_occ.upload(occ, n));
  G2_TRY(d_field.out(field, n));
  G2_TRY(wa.alloc(n));
  G2_TRY(wb.alloc(n));
  G2_TRY(launch_sdf_from_occupancy(nx, ny, nz, d_occ.p, cell, wa.p, wb.p, d_field.p, nullptr));
  return fetch_all(d_field);
}

int gpmp2mi_sdf_create_from_occupancy(int dim, const double origin[3], double cell, int nx, int ny, int nz,
                                      const double* occ, int layout, gpmp2mi_sdf** out) {
  G2_CHECK(out && origin && occ, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  if (dim == 2) nz = 1;
  G2_CHECK(layout == GPMP2MI_SDF_LAYOUT_ZYX || layout == GPMP2MI_SDF_LAYOUT_GTSAM, GPMP2MI_ERR_INVALID,
           "unknown voxel layout");
  std::unique_ptr<gpmp2mi_sdf> s;
  G2_TRY(sdf_alloc(dim, origin, cell, nx, ny, nz, s));
  const size_t n = (size_t)nx * ny * nz;
  std::vector<double> tmp;
  DevBuf<double> d_occ;
  DevBuf<int> wa, wb;
  G2_TRY(d_occ.upload(to_zyx(occ, layout, nx, ny, nz, tmp), n));
  G2_TRY(wa.alloc(n));
  G2_TRY(wb.alloc(n));
  G2_TRY(launch_sdf_from_occupancy(nx, ny, nz, d_occ.p, cell, wa.p, wb.p, s->plain, nullptr));
  G2_TRY(launch_sdf_pack(s->h, s->cells, nullptr));
  G2_HIP(hipStreamSynchronize(nullptr));
  *out = s.release();
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_get_field(const gpmp2mi_sdf* s, int* dim, int* nx, int* ny, int* nz, double origin[3],
                          double* cell, double* field) {
  G2_CHECK(s, GPMP2MI_ERR_INVALID, "null argument");
  if (dim) *dim = s->h.dim;
  if (nx) *nx = s->h.nx;
  if (ny) *ny = s->h.ny;
  if (nz) *nz = s->h.nz;
  if (origin) origin[0] = s->h.ox, origin[1] = s->h.oy, origin[2] = s->h.oz;
  if (cell) *cell = s->h.cell;
  if (field)
    G2_HIP(hipMemcpy(field, s->plain, (size_t)s->h.nx * s->h.ny * s->h.nz * sizeof(double), hipMemcpyDeviceToHost));
  return GPMP2MI_OK;
}

int gpmp2mi_sdf_read_vol(const char* filename_pre, gpmp2mi_sdf** out) {
  G2_CHECK(filename_pre && out, GPMP2MI_ERR_INVALID, "null argument");
  *out = nullptr;
  const std::string pre(filename_pre);
  std::ifstream head(pre + ".vol.head");
  G2_CHECK(head.is_open(), GPMP2MI_ERR_INVALID, "cannot open " + pre + ".vol.head");
  long long cols = 0, rows = 0, nz = 0;
  double origin[3] = {0, 0, 0}, res = 0;
  head >> cols >> rows >> nz >> origin[0] >> origin[1] >> origin[2] >> res;
  G2_CHECK(!head.fail() && cols > 0 && rows > 0 && nz > 0 && res > 0, GPMP2MI_ERR_INVALID, "malformed " + pre + ".vol.head");
  std::ifstream data(pre + ".vol.data");
  G2_CHECK(data.is_open(), GPMP2MI_ERR_INVALID, "cannot open " + pre + ".vol.data");
  // x outermost, then y, then z (fileUtils.cpp:48-55)
  std::vector<double> zyx((size_t)cols * rows * nz);
  for (long long x = 0; x < cols; x++)
    for (long long y = 0; y < rows; y++)
      for (long long z = 0; z < nz; z++) {
        double v;
        data >> v;
        G2_CHECK(!data.fail(), GPMP2MI_ERR_INVALID, "short or malformed " + pre + ".vol.data");
        zyx[((size_t)z * rows + y) * cols + x] = v;
      }
  return gpmp2mi_sdf_create(3, origin, res, (int)cols, (int)rows, (int)nz, zyx.data(), GPMP2MI_SDF_LAYOUT_ZYX, out);
}
void gpmp2mi_sdf_destroy(gpmp2mi_sdf* s) { delete s; }

int gpmp2mi_sdf_query(const gpmp2mi_sdf* s, int M, const double* pts, double* dist, double* grad, int* inr) {
  G2_CHECK(s && pts && dist && M >= 0, GPMP2MI_ERR_INVALID, "null argument");
  if (M == 0) return GPMP2MI_OK;
  G2_TRY(ensure_device());
  DevBuf<double> dp, dd, dg;
  DevBuf<int> di;
  G2_TRY(dp.upload(pts, (size_t)M * s->h.dim));
  G2_TRY(dd.out(dist, M));
  if (grad) G2_TRY(dg.out(grad, (size_t)M * s->h.dim));
  if (inr) G2_TRY(di.out(inr, M));
  G2_TRY(launch_sdf_query(s->h, M, dp.p, dd.p, dg.p, di.p, nullptr));
  return fetch_all(dd, dg, di);
}

// -------------------------------------------------------------------------------------------- settings
void gpmp2mi_settings_default(gpmp2mi_settings* s, int dof) {
  std::memset(s, 0, sizeof(*s));
  s->dof = dof;
  s->total_step = 10;
  s->total_time = 1.0;
  s->conf_prior_sigma = 0.0001;
  s->vel_prior_sigma = 0.0001;
  s->epsilon = 0.2;
  s->cost_sigma = 0.1;
  s->obs_check_inter = 5;
  s->opt_type = GPMP2MI_OPT_DOGLEG;
  s->final_iter_no_increase = 1;
  s->rel_thresh = 1e-2;
  s->max_iter = 50;
}
void gpmp2mi_graph_opts_default(gpmp2mi_graph_opts* o) {
  std::memset(o, 0, sizeof(*o));
  o->lm_lambda_initial = 100.0;
  o->lm_lambda_factor = 10.0;
  o->lm_lambda_upper = 1e5;
  o->lm_lambda_lower = 0.0;
  o->lm_min_model_fidelity = 1e-3;
  o->dogleg_delta_initial = 0.2;
  o->abs_error_tol = 1e-5;
  o->error_tol = 0.0;
}

}  // extern "C"
