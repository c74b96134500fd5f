// selfpair.hip -- the self-collision table of a plan (include/gpmp2mi.h "self-collision table in a plan"): the setter
// that turns a gpmp2mi_self_pairs table into the plan's own records, and the count.  Kernel: selfpair_kernels.hip; the
// factor inside a plan is launched by plan_linearize (plan_run.hip).
#include <cmath>

#include "host.h"

using namespace g2;

extern "C" {

int gpmp2mi_plan_set_self_pairs(gpmp2mi_plan* p, const gpmp2mi_self_pairs* t) {
  G2_CHECK(p, GPMP2MI_ERR_INVALID, "null plan");
  PlanExtras& ex = p->ex;
  G2_CHECK(ex.sp_cap > 0, GPMP2MI_ERR_INVALID, "the plan was created without room for a self-collision table");
  const int P = t ? t->P : 0;
  G2_CHECK(P <= ex.sp_cap, GPMP2MI_ERR_INVALID, "more pairs than the plan was created with room for");
  std::vector<SelfPairRec> rec(P);
  if (P > 0) {
    const RobotDev& h = p->robot->h;
    G2_CHECK(t->S == h.nr_spheres && t->dof == h.dof && t->kind == h.kind, GPMP2MI_ERR_INVALID,
             "the pair table was made for another robot (sphere count / dof / kind)");
    std::vector<double> radius(h.nr_spheres);
    for (int s = 0; s < h.nr_spheres; s++) radius[h.sph_orig[s]] = h.sph_r[s];
    for (int i = 0; i < P; i++) {
      const double* row = t->data.data() + (size_t)4 * i;
      G2_CHECK(std::isfinite(row[2]), GPMP2MI_ERR_INVALID, "pair " + std::to_string(i) + ": epsilon is not finite");
      G2_CHECK(std::isfinite(row[3]) && row[3] > 0, GPMP2MI_ERR_INVALID,
               "pair " + std::to_string(i) + ": sigma is not finite or not positive");
      // ids were checked when the table was made; cen / Jc are in the caller's sphere order
      rec[i].a = (int)row[0];
      rec[i].b = (int)row[1];
      rec[i].total_eps = radius[rec[i].a] + radius[rec[i].b] + row[2];
      rec[i].w = 1.0 / (row[3] * row[3]);
    }
  }
  G2_PLAN_LIVE(p);
  if (P > 0) G2_HIP(hipMemcpy(ex.sp_rec, rec.data(), (size_t)P * sizeof(SelfPairRec), hipMemcpyHostToDevice));
  ex.sp_P = P;
  return GPMP2MI_OK;
}

int gpmp2mi_plan_self_pairs_count(const gpmp2mi_plan* p) { return p ? p->ex.sp_P : -1; }

}  // extern "C"
