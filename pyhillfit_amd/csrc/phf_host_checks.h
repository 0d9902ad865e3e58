// phf_host_checks.h — the argument checks the streaming analyses' C-ABI entries share (host side only).  `who` is the entry's name,
// `family` the analysis ("waic", "ppc", ..) where the text names its phf_<family>_workspace_bytes().  Every check returns PHF_OK or
// fails with PHF_ERR_INVALID_ARGUMENT and the reason in the error buffer; an entry calls them in the order it documents, the first
// fault decides the message.
#ifndef PHF_HOST_CHECKS_H
#define PHF_HOST_CHECKS_H

#include <initializer_list>

#include "phf_common.h"

// every dimension >= 1; `names` is how the text lists them ("num_problems, stride and num_chains")
inline int phf_check_positive(const char* who, const char* names, std::initializer_list<int> dims) {
  for (const int d : dims)
    if (d < 1) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: %s must be positive", who, names);
  return PHF_OK;
}

// the caller's block counts (as doubles: they may overflow an int), every one within a launch grid's 2^31 - 1
inline int phf_check_grid(const char* who, std::initializer_list<double> blocks) {
  for (const double b : blocks)
    if (b > 2147483647.0) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: launch grid too large (fewer problems per workspace)", who);
  return PHF_OK;
}

inline int phf_check_row_window(const char* who, int64_t num_rows, int64_t first_row, int64_t total_rows) {
  if (total_rows < 1 || num_rows < 0 || first_row < 0 || first_row + num_rows > total_rows)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: rows [first_row, first_row + num_rows) must lie in [0, total_rows)", who);
  return PHF_OK;
}

// `rule` words what the stride has to hold ("must be >= num_columns", "is smaller than the columns the likelihood reads")
inline int phf_check_row_stride(const char* who, int row_stride_cols, int needed_cols, const char* rule) {
  if (row_stride_cols < needed_cols) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: row_stride_cols %s", who, rule);
  return PHF_OK;
}

inline int phf_check_workspace(const char* who, const char* family, const void* workspace, size_t workspace_bytes, size_t need) {
  if (!workspace) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null workspace", who);
  if (workspace_bytes < need)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: workspace smaller than phf_%s_workspace_bytes()", who, family);
  return PHF_OK;
}

// the body of a phf_<family>_init after its shape checks: the workspace is there, large enough and ordinary device memory; its first
// zero_bytes are cleared on the stream
inline int phf_init_workspace(const char* who, const char* family, void* workspace, size_t workspace_bytes, size_t need, size_t zero_bytes,
                              void* stream) {
  int rc = phf_check_workspace(who, family, workspace, workspace_bytes, need);
  if (rc != PHF_OK) return rc;
  char what[96];
  std::snprintf(what, sizeof what, "%s: workspace", who);
  if ((rc = phf_require_device_memory(workspace, what)) != PHF_OK) return rc;
  if (hipMemsetAsync(workspace, 0, zero_bytes, static_cast<hipStream_t>(stream)) != hipSuccess) return phf_check_launch(who);
  return PHF_OK;
}

// the pointwise points: all arrays there, stride >= 1 (and <= max_stride where that is > 0), one row per problem (num_problems 0: any)
inline int phf_check_points(const char* who, const phf_pointwise_points* pts, int num_problems, int max_stride) {
  if (!pts || !pts->ln_conc || !pts->response || !pts->tag || !pts->count) return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: null points", who);
  if (pts->stride < 1 || pts->num_problems < 1 || (num_problems > 0 && pts->num_problems != num_problems))
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the points must have stride >= 1 and one row per problem (%d rows, %d problems)", who,
                     pts->num_problems, num_problems);
  if (max_stride > 0 && pts->stride > max_stride)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: at most %d points per problem (stride %d)", who, max_stride, pts->stride);
  return PHF_OK;
}

// likelihood 1 | 2: the single-level model; 3: hierarchical, with num_expts experiments
inline int phf_check_likelihood(const char* who, int likelihood, int num_expts) {
  if (likelihood < 1 || likelihood > 3)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: likelihood must be 1, 2 (single-level model) or 3 (hierarchical)", who);
  if (likelihood == 3 && num_expts < 1)
    return phf_failf(PHF_ERR_INVALID_ARGUMENT, "%s: the hierarchical likelihood needs num_expts >= 1", who);
  return PHF_OK;
}

#endif  // PHF_HOST_CHECKS_H
