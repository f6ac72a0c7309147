// Thread-local error text + ABI version.
#include "common.h"

namespace gnpde {
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace gnpde

namespace gnpde { int g_tune[GNPDE_TUNE_COUNT] = {0}; int g_agg_fold_launch = 0; }

extern "C" int gnpde_tune(int32_t key, int32_t value) {
  GNPDE_CHECK_ARG(key >= 0 && key < gnpde::GNPDE_TUNE_COUNT, GNPDE_EINVAL, "tune: bad key %d", key);
  const bool retired = key == gnpde::GNPDE_TUNE_RETIRED_0 || key == gnpde::GNPDE_TUNE_RETIRED_8 || key == gnpde::GNPDE_TUNE_RETIRED_13;
  GNPDE_CHECK_ARG(!retired || value == 0, GNPDE_EINVAL, "tune: key %d is retired: the variant %d it selected was removed (it was last in c657da7; "
                  "its measurements are in profiles/ and DESIGN.md)", key, value);
  GNPDE_CHECK_ARG(key != gnpde::GNPDE_TUNE_KNN_VARIANT || value != 1, GNPDE_EINVAL, "tune: value 1 of key %d is retired: the 32-float K "
                  "chunks of the neighbour search were removed, slower at both shapes (profiles/knn_ab.jsonl)", key);
  gnpde::g_tune[key] = value;
  return 0;
}

extern "C" int gnpde_agg_fold_launch(int32_t keep) {
  GNPDE_CHECK_ARG(keep == 0 || keep == 1, GNPDE_EINVAL, "agg_fold_launch: %d is neither 0 nor 1", keep);
  gnpde::g_agg_fold_launch = keep;
  return 0;
}

extern "C" int gnpde_abi_version(void) { return GNPDE_ABI_VERSION; }
extern "C" const char* gnpde_last_error(void) { return gnpde::g_err; }
