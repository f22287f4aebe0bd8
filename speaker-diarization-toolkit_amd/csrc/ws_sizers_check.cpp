// Host-side soundness check of the workspace sizers (make ws_sizers_check): every sdk_*_workspace_bytes at its smallest accepted arguments, its
// largest, and one set just outside, with the library's host code built under UBSan + ASan.  No GPU, no Python: the sizers are host functions
// and measure their layouts on a null base (csrc/workspace.hpp), which must never form a pointer from it.  Exit status 0 and no sanitizer
// report: sound.  The values themselves are pinned by tests/test_workspace_sizers_cpu.py; here accepted means > 0 and refused means 0.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/sdk_hip.h"

static int failures = 0;
static void expect(const char* what, size_t got, bool accepted) {
  if ((got > 0) == accepted) return;
  printf("%s = %zu: expected %s\n", what, got, accepted ? "a size" : "a refusal (0)");
  ++failures;
}
// smallest accepted, largest accepted, just outside
#define SIZER3(fn, small, large, outside)   \
  do {                                      \
    expect(#fn #small, fn small, true);     \
    expect(#fn #large, fn large, true);     \
    expect(#fn #outside, fn outside, false); \
  } while (0)

int main() {
  const int BIG_B = 1 << 20, BIG_T = 2047;                    // B * T just below 2^31: the largest batch the forwards take
  SIZER3(sdk_fbank_workspace_bytes, (1, 1), (4096, 160000), (0, 1));
  SIZER3(sdk_se_workspace_bytes, (1, 1, 1), (65536, 1024, 128), (1, 0, 1));
  SIZER3(sdk_samples_runs_workspace_bytes, (0), ((1ll << 30) - 1), (1ll << 30));
  SIZER3(sdk_samples_score_workspace_bytes, (0, 0, 64), ((1 << 24) - 1, (1 << 24) - 1, 512), (1 << 24, 0, 64));
  SIZER3(sdk_smooth_turns_workspace_bytes, (0), ((1ll << 30) - 1), (-1));
  SIZER3(sdk_vbx_workspace_bytes, (1, 64, 1), (65536, 128, 65536), (65537, 64, 1));
  SIZER3(sdk_vbx_hmm_workspace_bytes, (1, 64, 1), (65536, 128, 65536), (1, 64, 0));
  SIZER3(sdk_plda_fit_stats_workspace_bytes, (1, 1, 0, 0), (1 << 24, 512, 1 << 24, 1), ((1 << 24) + 1, 512, 0, 1));
  SIZER3(sdk_kmeans_rows_workspace_bytes, (1, 64, 1), (65536, 512, 64), (10, 64, 11));
  SIZER3(sdk_cohort_stats_workspace_bytes, (0, 1, 1), (2147483647, 1 << 20, 1 << 20), (10, (1 << 20) + 1, 5));
  SIZER3(sdk_plda_enroll_workspace_bytes, (0, 1), (1 << 22, 1 << 20), ((1 << 22) + 1, 1));
  SIZER3(sdk_plda_score_workspace_bytes, (0, 1, 1), (65536, 1 << 20, 4), (65537, 1, 1));
  SIZER3(sdk_trial_calib_workspace_bytes, (1, 1, 0), (1 << 20, 1 << 20, 2147483647), (0, 1, 0));
  SIZER3(sdk_affinity_workspace_bytes, (1, 1), (1 << 20, 1 << 20), (0, 1));
  SIZER3(sdk_affinity_matvec_workspace_bytes, (1), (1 << 24), ((1 << 24) + 1));
  SIZER3(sdk_laplacian_topk_workspace_bytes, (1, 1), (1 << 24, 32), (1 << 24, 33));
  SIZER3(sdk_rows_gram_workspace_bytes, (1, 1), (1 << 24, 32), (0, 1));
  SIZER3(sdk_knn_reverse_workspace_bytes, (2, 1), (65536, 64), (1, 1));
  expect("sdk_stream_state_bytes(1, 1, 64)", (size_t)sdk_stream_state_bytes(1, 1, 64), true);
  expect("sdk_stream_state_bytes(1 << 20, 64, 512)", (size_t)sdk_stream_state_bytes(1 << 20, 64, 512), true);
  expect("sdk_stream_state_bytes(0, 1, 64)", (size_t)sdk_stream_state_bytes(0, 1, 64), false);

  sdk_ecapa_desc e;
  memset(&e, 0, sizeof(e));
  e.n_mels_padded = 128; e.channels = 1024; e.sub_channels = 128; e.scale = 8; e.se_channels = 128; e.attn_channels = 128; e.mfa_channels = 3072;
  e.embed_dim = 192; e.n_blocks = 3; e.kernel0 = 5;
  for (int precision = 0; precision <= 2; ++precision) {
    e.precision = precision;
    SIZER3(sdk_ecapa_workspace_bytes, (&e, 1, 1), (&e, BIG_B, BIG_T), (&e, BIG_B, BIG_T + 1));
    if (precision != 1) SIZER3(sdk_ecapa_masked_workspace_bytes, (&e, 1, 1, 1), (&e, BIG_B, BIG_T, 8), (&e, 1, 1, 9));
    else expect("sdk_ecapa_masked_workspace_bytes(precision 1)", sdk_ecapa_masked_workspace_bytes(&e, 1, 1, 1), false);
  }
  expect("sdk_ecapa_workspace_bytes(NULL, 1, 1)", sdk_ecapa_workspace_bytes(nullptr, 1, 1), false);

  sdk_xvector_desc x;
  memset(&x, 0, sizeof(x));
  x.n_frame_layers = 5; x.n_feats = 128; x.embed_dim = 512;
  for (int l = 0; l < 5; ++l) { x.cout[l] = l == 4 ? 1536 : 512; x.cin[l] = l ? x.cout[l - 1] : 128; x.kernel[l] = 1; x.dilation[l] = 1; }
  for (int precision = 0; precision <= 2; ++precision) {
    x.off[62] = precision;
    SIZER3(sdk_xvector_workspace_bytes, (&x, 1, 1), (&x, BIG_B, BIG_T), (&x, 0, 1));
  }

  sdk_resnet_desc r;
  memset(&r, 0, sizeof(r));
  r.n_feats = 80; r.embed_dim = 256; r.n_layers = 4;
  const int blocks[4] = {3, 4, 6, 3}, width[4] = {32, 64, 128, 256};
  for (int l = 0; l < 4; ++l) { r.blocks[l] = blocks[l]; r.width[l] = width[l]; }
  SIZER3(sdk_resnet_workspace_bytes, (&r, 1, 1), (&r, BIG_B, BIG_T), (&r, BIG_B, BIG_T + 1));
  SIZER3(sdk_resnet_masked_workspace_bytes, (&r, 1, 1, 1), (&r, BIG_B, BIG_T, 2047), (&r, 1, 1, 0));

  sdk_segmentation_desc s;
  memset(&s, 0, sizeof(s));
  SIZER3(sdk_segmentation_workspace_bytes, (&s, 1, 991), (&s, 1 << 20, 160000), (&s, 1, 990));

  // the linkages: one problem of one row; as many problems of 65536 rows as int32 offsets hold; a problem of 65537 rows
  const int32_t one[2] = {0, 1}, over[2] = {0, 65537};
  std::vector<int32_t> big(32769);
  for (int g = 0; g < 32768; ++g) big[g] = 65536 * g;
  big[32768] = 2147483647;
  SIZER3(sdk_centroid_linkage_workspace_bytes, (one, 1, 1), (big.data(), 32768, 2048), (over, 1, 64));
  SIZER3(sdk_linked_linkage_workspace_bytes, (one, 1, 1), (big.data(), 32768, 2048), (one, 0, 64));

  printf("ws_sizers_check: %d failure%s\n", failures, failures == 1 ? "" : "s");
  return failures != 0;
}
