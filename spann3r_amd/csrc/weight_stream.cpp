// Which launches of the per-frame chain read their weights with the streaming (non-temporal) policy: csrc/common.h ld_w16 /
// SP3_AUX_STREAM on the device side, this table on the host side.  The policy is no descriptor field: sp3_gemm_plan's answers, the
// launch census and every result are the same under all modes.
#include <atomic>
#include <stdlib.h>
#include "common.h"

namespace {

// The shipped table (mode 1), per family and instance: decided in the model, not in a micro-benchmark that replays one launch on warm
// weights (there the default policy always wins) -- DESIGN.md section 6 "weight cache policy" has the numbers of every entry.
// An instance that is not listed uses the default policy.
struct Entry { int family, instance; bool stream; };
const Entry kTable[] = {
    // lean 196-row GEMMs (gemm_sm.hip sm_kernel), by tile id
    {SP3_WF_GEMM_SM, 30, true},   // value encoder / encoder-step q/k/v
    {SP3_WF_GEMM_SM, 31, true},   // decoder q/k/v + cross k/v pair
    {SP3_WF_GEMM_SM, 32, true},   // value encoder fc1
    {SP3_WF_GEMM_SM, 33, true},   // decoder fc1
    {SP3_WF_GEMM_SM, 42, true},   // key MLP hidden (split A)
    {SP3_WF_GEMM_SM, 39, true},   // decoder_embed
    {SP3_WF_GEMM_SM, 34, true},   // value encoder proj, value_out
    {SP3_WF_GEMM_SM, 35, true},   // value encoder fc2
    {SP3_WF_GEMM_SM, 36, true},   // decoder proj / cross proj
    {SP3_WF_GEMM_SM, 37, true},   // decoder fc2
    {SP3_WF_GEMM_SM, 38, true},   // key MLP out
    // (tile 43, the memory read's score GEMM: its W is the bank's K-hat, re-read every step -- no streaming variant exists)
    // small-map 3x3 convolutions of the DPT heads (gemm_sm.hip conv_sm_body), by tile id
    {SP3_WF_CONV_SM, 40, true},
    {SP3_WF_CONV_SM, 41, true},
    // the q projection inside the cross-attention launch (attention.hip attn_qproj): the 13 query blocks of a head re-read its 96 KB of
    // Wq from L2 -- the headline is 0.3 % faster with these loads on the default policy
    {SP3_WF_ATTN_QPROJ, 0, false},
    // wide 3x3 convolution (conv.hip conv3x3_wide_kernel), by NF: every pixel tile re-reads the weight panel of its output channels
    // (28 workgroups per panel at 56 x 56, 98 at 112 x 112) -- streaming costs the kernel 15-17 %
    {SP3_WF_CONV_WIDE, 2, false},
    {SP3_WF_CONV_WIDE, 4, false},
};

int env_mode() {
  const char* e = getenv("SP3_W_STREAM");
  if (e && e[0] >= '0' && e[0] <= '2' && e[1] == 0) return e[0] - '0';
  return 1;
}

std::atomic<int>& mode() {
  static std::atomic<int> m(env_mode());
  return m;
}

}  // namespace

bool sp3_weight_streams(int family, int instance) {
  const int m = mode().load(std::memory_order_relaxed);
  if (m == 0) return false;
  if (m == 2) return true;
  for (const Entry& e : kTable)
    if (e.family == family && e.instance == instance) return e.stream;
  return false;
}

extern "C" int sp3_weight_stream_set(int m) {
  SP3_CHECK(m >= 0 && m <= 2, "sp3_weight_stream_set: mode %d (0 default policy, 1 the library's table, 2 every streaming variant)", m);
  mode().store(m, std::memory_order_relaxed);
  return 0;
}

extern "C" int sp3_weight_stream_get(void) { return mode().load(std::memory_order_relaxed); }
