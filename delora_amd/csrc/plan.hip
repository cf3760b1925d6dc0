// dl_conv_plan_describe: what the convolution dispatch would launch.  The entry points themselves run, on the plan sink of common.h /
// abi.hip (every launch becomes a record), so the answer is the dispatch code's own, not a restatement of it.
#include <stdint.h>

#include "common.h"

/* see include/delora_hip.h */
extern "C" int dl_conv_plan_describe(int32_t op, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize,
                                     int32_t stride_h, int32_t stride_w, int32_t mode, int32_t cu_count, char* buf, size_t buf_bytes) {
  if (!buf || buf_bytes < 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_conv_plan_describe: no buffer");
  if (dtype != DL_DTYPE_F32 && dtype != DL_DTYPE_F16 && dtype != DL_DTYPE_BF16)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_conv_plan_describe: bad dtype %d", dtype);
  buf[0] = 0;
  DlPlanSink sink{buf, buf_bytes, 0, cu_count};
  // operands that are never dereferenced: the entry points check them for null and hand them to launches that do not happen
  void* const p = (void*)(uintptr_t)4096;
  const bool half = dtype != DL_DTYPE_F32;
  dl_wgrad_layer layer{p, p, (float*)p, N, H, W, C, K, ksize, stride_h, stride_w};
  g_dl_plan = &sink;
  int rc;
  switch (op) {
    case DL_PLAN_CONV:
      rc = half ? dl_conv2d_nhwc_h(p, p, p, nullptr, nullptr, N, H, W, C, K, ksize, stride_h, stride_w, mode, dtype, 0, 0, nullptr)
                : dl_conv2d_nhwc_f32((const float*)p, (const float*)p, (float*)p, nullptr, nullptr, N, H, W, C, K, ksize, stride_h, stride_w, mode, 0, 0, nullptr);
      break;
    case DL_PLAN_DGRAD_STRIDED:
      rc = half ? dl_conv2d_dgrad_strided_nhwc_h(p, p, p, nullptr, nullptr, N, H, W, K, C, ksize, stride_h, stride_w, mode, dtype, 0, 0, (float*)p, nullptr)
                : dl_conv2d_dgrad_strided_nhwc_f32((const float*)p, (const float*)p, (float*)p, nullptr, nullptr, N, H, W, K, C, ksize, stride_h, stride_w, mode, 0, 0, (float*)p, nullptr);
      break;
    case DL_PLAN_WINO_CONV:
      rc = half ? dl_fail(DL_ERR_UNSUPPORTED, "dl_conv_plan_describe: the Winograd kernels are fp32")
                : dl_wino_conv3x3_nhwc_f32((const float*)p, (const float*)p, (float*)p, nullptr, nullptr, N, H, W, C, K, 0, 0, mode ? nullptr : p, nullptr);
      break;
    case DL_PLAN_WGRAD:
      rc = half ? dl_conv2d_wgrad_nhwc_h(p, p, (float*)p, p, N, H, W, C, K, ksize, stride_h, stride_w, dtype, nullptr)
                : dl_conv2d_wgrad_nhwc_f32((const float*)p, (const float*)p, (float*)p, p, N, H, W, C, K, ksize, stride_h, stride_w, nullptr);
      break;
    case DL_PLAN_WGRAD_BATCH:
      rc = half ? dl_conv2d_wgrad_batch_nhwc_h(&layer, 1, p, dtype, nullptr) : dl_conv2d_wgrad_batch_nhwc_f32(&layer, 1, p, nullptr);
      break;
    case DL_PLAN_WINO_WGRAD:
      rc = half ? dl_fail(DL_ERR_UNSUPPORTED, "dl_conv_plan_describe: the Winograd kernels are fp32")
                : dl_wino_wgrad3x3_nhwc_f32((const float*)p, (const float*)p, (float*)p, p, N, H, W, C, K, nullptr);
      break;
    case DL_PLAN_WINO_WGRAD_BATCH:
      rc = half ? dl_fail(DL_ERR_UNSUPPORTED, "dl_conv_plan_describe: the Winograd kernels are fp32")
                : dl_wino_wgrad3x3_batch_nhwc_f32(&layer, 1, p, nullptr);
      break;
    default:
      rc = dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_conv_plan_describe: unknown op %d", op);
  }
  g_dl_plan = nullptr;
  if (rc) return rc;
  if (sink.len + 1 > buf_bytes) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_conv_plan_describe: the text needs %zu bytes", sink.len + 1);
  return DL_OK;
}
