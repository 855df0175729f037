// Species occurrence heat-map grids of the range-filter meta-model (api_predict.cpp bnhip_range_heatmap): the kernels that turn a grid of
// cell centres into model rows and keep one output column of every row.
#pragma once
#include <hip/hip_runtime.h>

namespace bnhip {

// Rows g0 .. g0+n-1 of the grid, row g = week index wi * n_cells + cell c, into rows[n][3] = {lat_c, lon_c, 1 + wi * stride}
// (coords = [n_cells][2] lat / lon pairs, used exactly as given).
void launch_heatmap_rows(const float* coords, int n_cells, int stride, int g0, int n, float* rows, hipStream_t s);

// Pruned tail: out[r] = act(sum_k a[r][k] * w[k] + bias) for n rows of the penultimate activation a[n][K] (w = the species'
// weight row of the final dense layer, bias may be NULL).  One fp32 sum per row in a fixed order.
void launch_heatmap_column(const float* a, int K, const float* w, const float* bias, int act, int n, float* out, hipStream_t s);

// Gather tail: out[r] = logits[r][col] for n rows of logits[n][n_classes].
void launch_heatmap_gather(const float* logits, int n_classes, int col, int n, float* out, hipStream_t s);

}  // namespace bnhip
