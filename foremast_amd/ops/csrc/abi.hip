// ABI introspection for the ctypes binding (sizeof / offsetof of the arg structs).
#include <hip/hip_runtime.h>
#include "args.h"

#define FM_OFF(S, f) if (!__builtin_strcmp(field, #f)) return (long long)offsetof(S, f)

extern "C" long long fm_abi_sizeof(const char* name) {
  if (!__builtin_strcmp(name, "DetectArgs")) return sizeof(DetectArgs);
  if (!__builtin_strcmp(name, "SmoothArgs")) return sizeof(SmoothArgs);
  if (!__builtin_strcmp(name, "RankArgs")) return sizeof(RankArgs);
  if (!__builtin_strcmp(name, "WindowArgs")) return sizeof(WindowArgs);
  if (!__builtin_strcmp(name, "RobustArgs")) return sizeof(RobustArgs);
  if (!__builtin_strcmp(name, "BivArgs")) return sizeof(BivArgs);
  if (!__builtin_strcmp(name, "BivPairArgs")) return sizeof(BivPairArgs);
  if (!__builtin_strcmp(name, "MvnGroupArgs")) return sizeof(MvnGroupArgs);
  if (!__builtin_strcmp(name, "MvnFitStateArgs")) return sizeof(MvnFitStateArgs);
  if (!__builtin_strcmp(name, "MvnStateDetectArgs")) return sizeof(MvnStateDetectArgs);
  return -1;
}

extern "C" long long fm_abi_offsetof(const char* name, const char* field) {
  if (!__builtin_strcmp(name, "SmoothArgs")) { FM_OFF(SmoothArgs, det); FM_OFF(SmoothArgs, season_out); FM_OFF(SmoothArgs, grid); FM_OFF(SmoothArgs, head_dev); FM_OFF(SmoothArgs, season_hb); FM_OFF(SmoothArgs, nvalid_out); }
  if (!__builtin_strcmp(name, "DetectArgs")) { FM_OFF(DetectArgs, pw_scale); FM_OFF(DetectArgs, app_stats); FM_OFF(DetectArgs, ld_cur);
    FM_OFF(DetectArgs, threshold_low); FM_OFF(DetectArgs, hv_grid); FM_OFF(DetectArgs, hv_m); FM_OFF(DetectArgs, forecast);
    FM_OFF(DetectArgs, anom_count); FM_OFF(DetectArgs, anom_cap); FM_OFF(DetectArgs, thr_lut); FM_OFF(DetectArgs, lut_n);
    FM_OFF(DetectArgs, row_out); FM_OFF(DetectArgs, tick_min); FM_OFF(DetectArgs, shift_one_step); }
  if (!__builtin_strcmp(name, "RankArgs")) { FM_OFF(RankArgs, pvals); FM_OFF(RankArgs, alpha); FM_OFF(RankArgs, p_friedman); FM_OFF(RankArgs, pods_b); FM_OFF(RankArgs, z_crit); }
  if (!__builtin_strcmp(name, "WindowArgs")) { FM_OFF(WindowArgs, det); }
  if (!__builtin_strcmp(name, "RobustArgs")) { FM_OFF(RobustArgs, det); FM_OFF(RobustArgs, mad); FM_OFF(RobustArgs, sigma); }
  if (!__builtin_strcmp(name, "BivArgs")) { FM_OFF(BivArgs, eps); FM_OFF(BivArgs, app_stats); }
  if (!__builtin_strcmp(name, "BivPairArgs")) { FM_OFF(BivPairArgs, threshold); FM_OFF(BivPairArgs, anom_val); }
  if (!__builtin_strcmp(name, "MvnGroupArgs")) { FM_OFF(MvnGroupArgs, thr2); FM_OFF(MvnGroupArgs, contrib); FM_OFF(MvnGroupArgs, anom_val); FM_OFF(MvnGroupArgs, kmask); }
  if (!__builtin_strcmp(name, "MvnFitStateArgs")) { FM_OFF(MvnFitStateArgs, groups); FM_OFF(MvnFitStateArgs, dst); FM_OFF(MvnFitStateArgs, eps); FM_OFF(MvnFitStateArgs, chol); FM_OFF(MvnFitStateArgs, kmask); }
  if (!__builtin_strcmp(name, "MvnStateDetectArgs")) { FM_OFF(MvnStateDetectArgs, active); FM_OFF(MvnStateDetectArgs, ld_cur); FM_OFF(MvnStateDetectArgs, min_valid); FM_OFF(MvnStateDetectArgs, contrib); FM_OFF(MvnStateDetectArgs, anom_cap); FM_OFF(MvnStateDetectArgs, kmask); }
  return -1;
}
