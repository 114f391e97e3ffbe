// gps_item_rows.hip -- a pre-train / grounding row's facts from one item id (gfx950).
//
// Reference: what ScanBase._getitem_refer / _getitem_finalrefer look up per sample on the data-loader workers
// (data/datasets/base.py:348-417, :851-957): the item's scan, the position of its target among the scan's objects,
// cat2int[instance_type], its sentence, and np.random.choice of one of the scan's captions (base.py:851-856).  Here the
// items are resident (struct gps_item_table, the twin of gps_qa_questions) and one thread per row copies them out, so
// the batch is a (B,) tensor of item ids and the chain behind it -- gps_obj_select / _pred, gps_text_batch -- reads
// device tables only.  The rule is stated in include/gps_hip.h; tests/augdraw_cases.py restates it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dropout.h"
#include "gps_hip.h"

namespace gps_items {

constexpr int kBlock = 64;

__global__ __launch_bounds__(kBlock) void item_rows_kernel(int B, gps_item_table t, const int32_t *__restrict__ item_ids,
                                                           const int32_t *__restrict__ pick, uint64_t seed,
                                                           const uint64_t *seed_dev, int32_t *__restrict__ scan_range,
                                                           int32_t *__restrict__ prop_range, int32_t *__restrict__ tgt_obj,
                                                           int32_t *__restrict__ tgt_label, int32_t *__restrict__ sent_idx,
                                                           int32_t *__restrict__ cap_idx, int32_t *__restrict__ scan_idx) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int i = item_ids[b];
  int s = -1;
  if (i >= 0 && i < t.n_items) s = t.item_scan[i];
  if (s < 0 || s >= t.n_scans) {                 // an undefined row: empty ranges, no text
    scan_range[2 * b] = scan_range[2 * b + 1] = 0;
    prop_range[2 * b] = prop_range[2 * b + 1] = 0;
    tgt_obj[b] = 0;
    tgt_label[b] = 0;
    sent_idx[b] = -1;
    cap_idx[b] = -1;
    scan_idx[b] = -1;
    return;
  }
  scan_range[2 * b] = t.scan_range[2 * s];
  scan_range[2 * b + 1] = t.scan_range[2 * s + 1];
  prop_range[2 * b] = t.prop_range[2 * s];
  prop_range[2 * b + 1] = t.prop_range[2 * s + 1];
  tgt_obj[b] = t.item_tgt[i];
  tgt_label[b] = t.item_label[i];
  sent_idx[b] = t.item_sent[i];
  scan_idx[b] = s;
  int first = t.cap_first[s], last = t.cap_first[s + 1];         // clamped to the caption array
  first = first < 0 ? 0 : (first > t.n_caps ? t.n_caps : first);
  last = last < first ? first : (last > t.n_caps ? t.n_caps : last);
  const int n = last - first;
  if (n <= 0) {
    cap_idx[b] = t.default_caption;
    return;
  }
  int p;
  if (pick) {
    p = pick[b];
    if (p < 0 || p >= n) p = 0;
  } else {
    const uint64_t S = (seed + (seed_dev ? *seed_dev : 0ull)) + 5ull;
    p = (int)(gps_dropout::rng_u32(S, (uint64_t)b) % (uint32_t)n);
  }
  cap_idx[b] = t.cap_text[first + p];
}

}  // namespace gps_items

extern "C" int gps_item_rows(int B, const gps_item_table *items, const int32_t *item_ids, const int32_t *pick,
                             uint64_t seed, const uint64_t *seed_dev, int32_t *scan_range, int32_t *prop_range,
                             int32_t *tgt_obj, int32_t *tgt_label, int32_t *sent_idx, int32_t *cap_idx,
                             int32_t *scan_idx, gps_stream_t stream) {
  if (B < 0 || !items) return GPS_ERR_INVALID_ARGUMENT;
  const gps_item_table &t = *items;
  if (t.n_items < 0 || t.n_scans < 0 || t.n_caps < 0) return GPS_ERR_INVALID_ARGUMENT;
  if (t.n_items > 0 && (!t.item_scan || !t.item_tgt || !t.item_label || !t.item_sent)) return GPS_ERR_INVALID_ARGUMENT;
  if (t.n_scans > 0 && (!t.scan_range || !t.prop_range)) return GPS_ERR_INVALID_ARGUMENT;
  if (!t.cap_first || (t.n_caps > 0 && !t.cap_text)) return GPS_ERR_INVALID_ARGUMENT;
  if (B == 0) return GPS_OK;
  if (!item_ids || !scan_range || !prop_range || !tgt_obj || !tgt_label || !sent_idx || !cap_idx || !scan_idx)
    return GPS_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(gps_items::item_rows_kernel, dim3((B + gps_items::kBlock - 1) / gps_items::kBlock),
                     dim3(gps_items::kBlock), 0, (hipStream_t)stream, B, t, item_ids, pick, seed, seed_dev, scan_range,
                     prop_range, tgt_obj, tgt_label, sent_idx, cap_idx, scan_idx);
  return hipGetLastError() == hipSuccess ? GPS_OK : GPS_ERR_LAUNCH;
}
