// gps_text.hip -- the text side of a training batch on MI355X (gfx950): token gather, caption / sentence merge and the
// masked-LM / masked-object draws, from a corpus that was tokenised once and lives on the device.
//
// Reference (what this one entry replaces on the data-loader workers, per sample):
//   MaskDatasetWrapper.__getitem__   data/datasets/dataset_wrapper.py:38-111  tokenizer(sentence), tokenizer(scene_cap +
//                                                                             " " + sentence), the two masking calls
//   merge_tokens                     data/data_utils.py:50-60                 the pre-tokenised form of the same merge
//   random_word                      data/data_utils.py:76-104                per token: a draw, 80 / 10 / 10
//   random_point_cloud               data/data_utils.py:107-121               per object slot: a draw
//
// gps_text_batch   ONE launch, no atomics, no workspace, no host sync; every element of every output is written.
//   Grid: one workgroup of 256 threads (four waves) per text row, then one workgroup per 256 object slots.  A text row is
//   L + Ls positions (50 + 300 in the published configs): thread j takes positions j, j + 256, ..., so consecutive lanes
//   store consecutive int64 words (512 B per wave and store instruction).  The row's two texts are resolved with two
//   offset loads each (off[id], off[id + 1], wave-uniform), the concatenation caption ++ sentence by one comparison per
//   position -- no search.  Every load of a position (its token, its replay draws) is issued before the first branch
//   that depends on one of them (GPS_LOADS_ISSUED).
//
// The device draw law (no replay draws given), all in integers so that a numpy emulation is bit-equal:
//   S = effective_seed(seed, seed_dev);  T(x) = floor(x * 2^32) as a 64-bit number (2^32 at x = 1: every position);
//   token (r, t):  u = rng_u32(S, r * L + t), masked iff u < T(txt_mask_ratio); among the masked 10 u < 8 T -> mask_id,
//                  8 T <= 10 u < 9 T -> (uint64(rng_u32(S + 1, r * L + t)) * vocab_size) >> 32, else the id stays;
//   object (r, o): dropped iff rng_u32(S + 2, r * O + o) < T(pc_mask_ratio).
// The replay law (the reference's arithmetic in double on recorded draws) and the text rules are stated in
// include/gps_hip.h; tests/text_cases.py restates all of them in numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gps_dev.h"
#include "gps_dropout.h"
#include "gps_hip.h"

namespace gps_text {

constexpr int kBlock = 256;
constexpr int kMaxLen = 1 << 20;                // L, Ls, O above it: GPS_ERR_UNSUPPORTED

enum Mode { kGather = 0, kReplay = 1, kDevice = 2 };

struct Params {
  int n_texts, n_rows, L, Ls, scene_sent_cap;
  int cls_id, sep_id, mask_id, pad_id, vocab_size;
  long long n_tok, n_obj;                       // tokens in `tok`; n_obj_rows * O object slots
  double txt_ratio, pc_ratio;
  unsigned long long txt_thr, pc_thr;           // floor(ratio * 2^32): 2^32 at ratio 1
  unsigned long long seed;
  const unsigned long long *seed_dev;
  const int32_t *tok;
  const int64_t *off;
  const int32_t *sent_idx, *cap_idx;
  const uint8_t *obj_masks;
  const double *u_tok, *u_obj;
  const int32_t *rand_tok;
  int64_t *txt_ids, *txt_masks, *labels, *scene_ids, *scene_masks;
  uint8_t *obj_sem;
};

struct Seg {
  long long first, len;
};

// text `id` as a segment of `tok`; an id outside [0, n_texts), or offsets that leave the array, read as an empty text
__device__ __forceinline__ Seg segment(const Params &p, int id) {
  Seg s{0, 0};
  if (id < 0 || id >= p.n_texts) return s;
  const long long a = p.off[id], b = p.off[id + 1];
  if (a < 0 || b < a || b > p.n_tok) return s;
  s.first = a;
  s.len = b - a;
  return s;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void text_batch_kernel(const Params p) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= p.n_rows) {
    // ---- object slots: obj_sem_masks = obj_masks && !dropped -------------------------------------------------------
    const long long e = (long long)((int)blockIdx.x - p.n_rows) * kBlock + tid;
    if (e >= p.n_obj) return;
    const uint8_t have = p.obj_masks[e];
    bool drop = false;
    if (MODE == kReplay) {
      const double u = p.u_obj[e];
      GPS_LOADS_ISSUED();
      drop = u < p.pc_ratio;
    } else if (MODE == kDevice) {
      const unsigned long long S = gps_dropout::effective_seed(p.seed, p.seed_dev);
      drop = (unsigned long long)gps_dropout::rng_u32(S + 2ull, (unsigned long long)e) < p.pc_thr;
    }
    p.obj_sem[e] = (have != 0 && !drop) ? 1 : 0;
    return;
  }
  // ---- one text row --------------------------------------------------------------------------------------------------
  const int r = blockIdx.x;
  const int sid = p.sent_idx[r];
  const int cid = p.cap_idx ? p.cap_idx[r] : -1;
  const Seg s = segment(p, sid);
  const Seg c = segment(p, cid);
  const int L = p.L, Ls = p.cap_idx ? p.Ls : 0;
  const int n = (int)(s.len < (long long)(L - 2) ? s.len : (long long)(L - 2));          // sentence tokens kept
  const long long s_in = s.len < (long long)p.scene_sent_cap ? s.len : (long long)p.scene_sent_cap;
  const long long body_all = c.len + s_in;
  const int body = (int)(body_all < (long long)(p.Ls - 2) ? body_all : (long long)(p.Ls - 2));
  unsigned long long S = 0;
  if (MODE == kDevice) S = gps_dropout::effective_seed(p.seed, p.seed_dev);

  for (int j = tid; j < L + Ls; j += kBlock) {
    if (j < L) {
      const int t = j;
      const size_t e = (size_t)r * L + t;
      const bool from_text = t >= 1 && t <= n;
      int id = t == 0 ? p.cls_id : (t == n + 1 ? p.sep_id : p.pad_id);
      int tk = 0, rnd = 0;
      double u = 1.0;
      if (from_text) tk = p.tok[s.first + (t - 1)];
      if (MODE == kReplay) {
        u = p.u_tok[e];
        rnd = p.rand_tok[e];
      }
      GPS_LOADS_ISSUED();
      if (from_text) id = tk;
      const bool valid = t < n + 2;
      long long out = id, label = -1;
      if (valid && MODE == kReplay) {
        // random_word in Python's double arithmetic: prob < ratio, prob /= ratio, < 0.8, < 0.9
        if (u < p.txt_ratio) {
          label = id;
          const double q = u / p.txt_ratio;
          if (q < 0.8) out = p.mask_id;
          else if (q < 0.9) out = rnd;
        }
      } else if (valid && MODE == kDevice) {
        const unsigned long long h = gps_dropout::rng_u32(S, (unsigned long long)e);
        if (h < p.txt_thr) {
          label = id;
          if (10ull * h < 8ull * p.txt_thr) out = p.mask_id;
          else if (10ull * h < 9ull * p.txt_thr)
            out = (long long)(((unsigned long long)gps_dropout::rng_u32(S + 1ull, (unsigned long long)e) *
                               (unsigned long long)p.vocab_size) >> 32);
        }
      }
      p.txt_ids[e] = out;
      p.txt_masks[e] = valid ? 1 : 0;
      if (p.labels) p.labels[e] = label;
    } else {
      const int t = j - L;
      const size_t e = (size_t)r * p.Ls + t;
      const int k = t - 1;                       // index into caption ++ sentence
      const bool from_text = k >= 0 && k < body;
      int id = t == 0 ? p.cls_id : (k == body ? p.sep_id : p.pad_id);
      if (from_text) id = p.tok[(long long)k < c.len ? c.first + k : s.first + ((long long)k - c.len)];
      p.scene_ids[e] = id;
      p.scene_masks[e] = t < body + 2 ? 1 : 0;
    }
  }
}

}  // namespace gps_text

extern "C" int gps_text_batch(int n_texts, long long n_tok, const int32_t *tok, const int64_t *off, int n_rows,
                              const int32_t *sent_idx, const int32_t *cap_idx, int L, int Ls, int scene_sent_cap,
                              int cls_id, int sep_id, int mask_id, int pad_id, int vocab_size, int do_mask,
                              double txt_mask_ratio, double pc_mask_ratio, int n_obj_rows, int O,
                              const uint8_t *obj_masks, const double *u_tok, const int32_t *rand_tok,
                              const double *u_obj, uint64_t seed, const uint64_t *seed_dev, int64_t *txt_ids,
                              int64_t *txt_masks, int64_t *masked_lm_labels, int64_t *scene_txt_ids,
                              int64_t *scene_txt_masks, uint8_t *obj_sem_masks, gps_stream_t stream) {
  using namespace gps_text;
  if (L < 2 || Ls < 2 || n_texts < 0 || n_tok < 0 || n_rows < 0 || n_obj_rows < 0 || O < 0 || scene_sent_cap < 0 ||
      vocab_size < 1)
    return GPS_ERR_INVALID_ARGUMENT;
  // written so that a NaN ratio fails too
  if (!(txt_mask_ratio >= 0.0 && txt_mask_ratio <= 1.0) || !(pc_mask_ratio >= 0.0 && pc_mask_ratio <= 1.0))
    return GPS_ERR_INVALID_ARGUMENT;
  const long long n_obj = (long long)n_obj_rows * O;
  const bool replay = u_tok || rand_tok || u_obj;
  if (replay && (!u_tok || !rand_tok || (n_obj > 0 && !u_obj))) return GPS_ERR_INVALID_ARGUMENT;   // all or none
  if ((scene_txt_ids != nullptr) != (scene_txt_masks != nullptr)) return GPS_ERR_INVALID_ARGUMENT;
  if (n_rows == 0 && n_obj == 0) return GPS_OK;
  if (L > kMaxLen || Ls > kMaxLen || O > kMaxLen) return GPS_ERR_UNSUPPORTED;
  if (n_rows > 0) {
    if (!off || !sent_idx || !txt_ids || !txt_masks || (n_tok > 0 && !tok)) return GPS_ERR_INVALID_ARGUMENT;
    if (do_mask && !masked_lm_labels) return GPS_ERR_INVALID_ARGUMENT;
    if ((cap_idx != nullptr) != (scene_txt_ids != nullptr)) return GPS_ERR_INVALID_ARGUMENT;
  }
  if (n_obj > 0 && (!obj_masks || !obj_sem_masks)) return GPS_ERR_INVALID_ARGUMENT;
  const long long n_blocks = (long long)n_rows + (n_obj + kBlock - 1) / kBlock;
  if (n_blocks > 0x7fffffffll) return GPS_ERR_UNSUPPORTED;

  Params p;
  p.n_texts = n_texts; p.n_rows = n_rows; p.L = L; p.Ls = Ls; p.scene_sent_cap = scene_sent_cap;
  p.cls_id = cls_id; p.sep_id = sep_id; p.mask_id = mask_id; p.pad_id = pad_id; p.vocab_size = vocab_size;
  p.n_tok = n_tok; p.n_obj = n_obj;
  p.txt_ratio = txt_mask_ratio; p.pc_ratio = pc_mask_ratio;
  p.txt_thr = (unsigned long long)(txt_mask_ratio * 4294967296.0);
  p.pc_thr = (unsigned long long)(pc_mask_ratio * 4294967296.0);
  p.seed = seed; p.seed_dev = reinterpret_cast<const unsigned long long *>(seed_dev);
  p.tok = tok; p.off = off; p.sent_idx = sent_idx; p.cap_idx = n_rows > 0 ? cap_idx : nullptr;
  p.obj_masks = obj_masks; p.u_tok = u_tok; p.u_obj = u_obj; p.rand_tok = rand_tok;
  p.txt_ids = txt_ids; p.txt_masks = txt_masks; p.labels = masked_lm_labels;
  p.scene_ids = scene_txt_ids; p.scene_masks = scene_txt_masks; p.obj_sem = obj_sem_masks;

  const dim3 grid((unsigned int)n_blocks), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (!do_mask) hipLaunchKernelGGL(text_batch_kernel<kGather>, grid, block, 0, s, p);
  else if (replay) hipLaunchKernelGGL(text_batch_kernel<kReplay>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(text_batch_kernel<kDevice>, grid, block, 0, s, p);
  return gps_dev::launch_status();
}
