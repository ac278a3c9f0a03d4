// TEST INFRASTRUCTURE. The host's choice between the two forms of k_schur (schur_lean_form, csrc/gfbe_device.h) as the HIP-free half of
// the upload sees it, behind a C interface for tests/test_schur_form_host.py. No HIP call, no allocation.
#include "../ground-fusion2_amd/csrc/gfbe_upload.h"

extern "C" {

int sf_lean(int schur_groups, int vis_full, long long tot_lm) { return gfd::schur_lean_form(schur_groups, vis_full, tot_lm) ? 1 : 0; }
// the same on the batch-level members a plan leaves in a BatchDev (plan_to_batch): what launch_schur looks at
int sf_lean_of_plan(int B, int allreduce, int vis_full, int tot_lm) {
  gfd::UploadPlan p;
  p.B = B; p.cx.allreduce = allreduce != 0;
  p.schur_groups = B >= gfd::DENSE_SPLIT_MIN_B ? gfd::SCHUR_GROUPS : (allreduce ? gfd::NF : 2 * gfd::NF);      // (plan_upload's rule)
  p.vis_full = vis_full; p.tot_lm = tot_lm;
  gfd::BatchDev d;
  memset(&d, 0, sizeof d);
  gfd::plan_to_batch(p, d);
  return gfd::schur_lean_form(d.schur_groups, d.vis_full, d.tot_lm) ? 1 : 0;
}
int sf_groups() { return gfd::SCHUR_GROUPS; }

}  // extern "C"
