// Host side of the merged weight-gradient entry points, printed: workspace bytes, return code, error text and the plan text (kernel
// instantiation, grid, slab counts in launch order) of layer tables read from stdin.  Launches nothing and needs no GPU: the entry points
// run against a plan sink (csrc/common.h: DlPlanSink) with cu_count = 256 and dummy non-null pointers.
//
// stdin, one block per table:   family dtype n           family: direct | half | wino | pair      dtype: f32 | f16 | bf16
//                               N H W C K ksize stride_h stride_w        (n lines; none when n <= 0)
// stdout per table:             table <index> <family> <dtype> <n>
//                               bytes <workspace bytes>          [bytes_error <text>  when 0]
//                               rc <return code>                 [error <text>        when not 0]
//                               plan <one line per launch>
//                               end
// tests/test_wgrad_batch_plan_host.py compares this with tests/golden/wgrad_batch_plans.json.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../delora_amd/csrc/common.h"

int main() {
  char family[32], dtype_name[32];
  int n = 0, index = 0;
  std::vector<char> text(1 << 16);
  while (scanf("%31s %31s %d", family, dtype_name, &n) == 3) {
    std::vector<dl_wgrad_layer> layers(n > 0 ? n : 1);
    for (int i = 0; i < n; ++i) {
      dl_wgrad_layer& l = layers[i];
      if (scanf("%d %d %d %d %d %d %d %d", &l.N, &l.H, &l.W, &l.C, &l.K, &l.ksize, &l.stride_h, &l.stride_w) != 8) {
        fprintf(stderr, "wgrad_plan_dump: table %d: layer %d is not eight integers\n", index, i);
        return 2;
      }
      l.x = l.g = (const void*)(uintptr_t)4096;                 // never dereferenced: the sink replaces every launch
      l.dw = (float*)(uintptr_t)4096;
    }
    const std::string fam = family;
    const int dtype = !strcmp(dtype_name, "f16") ? DL_DTYPE_F16 : !strcmp(dtype_name, "bf16") ? DL_DTYPE_BF16 : DL_DTYPE_F32;
    if (fam != "direct" && fam != "half" && fam != "wino" && fam != "pair") {
      fprintf(stderr, "wgrad_plan_dump: table %d: unknown family %s\n", index, family);
      return 2;
    }
    DlPlanSink sink{text.data(), text.size(), 0, 256};
    text[0] = 0;
    g_dl_plan = &sink;
    void* ws = (void*)(uintptr_t)4096;
    size_t bytes = 0;
    std::string bytes_error;
    int rc = 0;
    if (fam == "direct") bytes = dl_conv2d_wgrad_batch_workspace_bytes(layers.data(), n);
    else if (fam == "half") bytes = dl_conv2d_wgrad_batch_h_workspace_bytes(layers.data(), n);
    else if (fam == "wino") bytes = dl_wino_wgrad3x3_batch_workspace_bytes(layers.data(), n);
    else bytes = dl_wino_strided_wgrad3x3_batch_workspace_bytes(layers.data(), n);
    if (!bytes) bytes_error = dl_last_error();
    if (fam == "direct") rc = dl_conv2d_wgrad_batch_nhwc_f32(layers.data(), n, ws, nullptr);
    else if (fam == "half") rc = dl_conv2d_wgrad_batch_nhwc_h(layers.data(), n, ws, dtype, nullptr);
    else if (fam == "wino") rc = dl_wino_wgrad3x3_batch_nhwc_f32(layers.data(), n, ws, nullptr);
    else rc = dl_wino_strided_wgrad3x3_batch_nhwc_f32(layers.data(), n, ws, nullptr);
    g_dl_plan = nullptr;
    printf("table %d %s %s %d\nbytes %zu\n", index, family, dtype_name, n, bytes);
    if (!bytes) printf("bytes_error %s\n", bytes_error.c_str());
    printf("rc %d\n", rc);
    if (rc) printf("error %s\n", dl_last_error());
    if (sink.len >= sink.cap) { fprintf(stderr, "wgrad_plan_dump: table %d: plan text of %zu bytes does not fit\n", index, sink.len); return 2; }
    for (const char* p = text.data(); *p;) {
      const char* e = strchr(p, '\n');
      const size_t m = e ? (size_t)(e - p) : strlen(p);
      printf("plan %.*s\n", (int)m, p);
      p += m + (e ? 1 : 0);
    }
    printf("end\n");
    ++index;
  }
  return 0;
}
