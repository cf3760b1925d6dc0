// Scan-to-scan odometry with no Python in it: a weight file written by delora_amd.deploy.native_infer.export_pose_net and a list of
// raw scans (float32 [3][N]: all x, all y, all z) go through dl_pose_net_prepare (once) and dl_odometry_push (once per scan), exactly
// as INTEGRATION.md section C describes for a C or C++ caller.  The counterpart of the reference's inference node (bin/run_rosnode.py)
// without ROS.
//
//   odometry_demo [--half bf16|f16] [--records <point_step> <off_x> <off_y> <off_z>] [--quality <half_rows> <half_cols> <epsilon_range> <min_neighbors>]
//                 <weights.dlpose> <out.txt> <scan0.bin> <scan1.bin> ...
//
// With --half the same program runs through the half-precision family (dl_pose_net_prepare_h, dl_odometry_push_h /
// dl_odometry_push_records_h): the fp32 weight file is converted once by the prepare call, the trunk runs in bf16 / fp16.
//
// With --records the scan files are raw point records as a sensor driver writes them (fp32 x, y, z at the three byte offsets of
// point_step-byte records; a KITTI .bin file is --records 16 0 4 8): they are uploaded as they are and pushed through
// dl_odometry_push_records with the reference node's filter (exactly-zero coordinates and ranges within 0.3 m are dropped inside
// the projection) -- nothing is filtered, compacted or transposed on the host.
//
// With --quality every push is followed by dl_odometry_quality with the given normal-estimation window (the shipped config is
// --quality 3 5 0.5 10): the program owns the two dl_scan_geometry records beside its two images, and every line ends with
//   quality <status> pairs <K> cov_diag <6 numbers>
// the status (0 fine, 1 at most six pairs, 2 unobservable), the pair count and the diagonal of the 6x6 covariance of the scan-to-scan
// transform (x, y, z, rotation about X, Y, Z; zeros unless the status is 0), which is also printed per push.
//
// One line per pair of consecutive scans:   <index> T <16 x 8 hex digits> pose <12 numbers>
// T = the fp32 bit patterns of the row-major 4x4 transform (previous -> current), pose = the first three rows of the accumulated
// T_0_t (the KITTI odometry format), accumulated in double.  Every HIP and dl_* status is checked; the first failure ends the
// program with a non-zero exit code.
#include <hip/hip_runtime.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

// the library's sources, as the other stand-alone programs of this directory take them
#include "../delora_amd/csrc/abi.hip"
#include "../delora_amd/csrc/project.hip"
#include "../delora_amd/csrc/conv.hip"
#include "../delora_amd/csrc/wino.hip"
#include "../delora_amd/csrc/stem.hip"
#include "../delora_amd/csrc/pose.hip"
#include "../delora_amd/csrc/heads.hip"
#include "../delora_amd/csrc/convh.hip"
#include "../delora_amd/csrc/infer.hip"
#include "../delora_amd/csrc/normals.hip"
#include "../delora_amd/csrc/nn.hip"
#include "../delora_amd/csrc/info.hip"

#define HIP_OK(call)                                                                                         \
  do {                                                                                                       \
    const hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) { fprintf(stderr, "odometry_demo: %s: %s\n", #call, hipGetErrorString(e_)); exit(2); } \
  } while (0)
#define DL_OK_OR_DIE(call)                                                                                   \
  do {                                                                                                       \
    const int rc_ = (call);                                                                                  \
    if (rc_ != 0) { fprintf(stderr, "odometry_demo: %s -> %d: %s\n", #call, rc_, dl_last_error()); exit(3); } \
  } while (0)

static void die(const std::string& what) {
  fprintf(stderr, "odometry_demo: %s\n", what.c_str());
  exit(1);
}

// ---------------------------------------------------------------------------------------------------------------------
// The JSON of the weight file's header: objects, arrays, strings without escapes beyond \" and \\, numbers, true / false / null.
struct Json {
  enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
  bool b = false;
  double num = 0.0;
  std::string str;
  std::vector<Json> items;
  std::map<std::string, Json> fields;
  const Json& at(const std::string& key) const {
    auto it = fields.find(key);
    if (kind != Object || it == fields.end()) die("weight file header: no field \"" + key + "\"");
    return it->second;
  }
  const Json& at(size_t i) const {
    if (kind != Array || i >= items.size()) die("weight file header: array too short");
    return items[i];
  }
  long long integer() const {
    if (kind != Number) die("weight file header: a number was expected");
    return (long long)num;
  }
};

struct JsonReader {
  const char* p;
  const char* end;
  void skip() { while (p < end && isspace((unsigned char)*p)) ++p; }
  void expect(char c) {
    skip();
    if (p >= end || *p != c) die(std::string("weight file header: '") + c + "' expected");
    ++p;
  }
  std::string string() {
    expect('"');
    std::string s;
    while (p < end && *p != '"') {
      if (*p == '\\' && p + 1 < end) ++p;
      s += *p++;
    }
    if (p >= end) die("weight file header: unterminated string");
    ++p;
    return s;
  }
  Json value() {
    skip();
    if (p >= end) die("weight file header: ends early");
    Json v;
    if (*p == '{') {
      v.kind = Json::Object;
      ++p; skip();
      if (p < end && *p == '}') { ++p; return v; }
      for (;;) {
        skip();
        const std::string key = string();
        expect(':');
        v.fields[key] = value();
        skip();
        if (p < end && *p == ',') { ++p; continue; }
        expect('}');
        return v;
      }
    }
    if (*p == '[') {
      v.kind = Json::Array;
      ++p; skip();
      if (p < end && *p == ']') { ++p; return v; }
      for (;;) {
        v.items.push_back(value());
        skip();
        if (p < end && *p == ',') { ++p; continue; }
        expect(']');
        return v;
      }
    }
    if (*p == '"') { v.kind = Json::String; v.str = string(); return v; }
    if (end - p >= 4 && !strncmp(p, "true", 4)) { v.kind = Json::Bool; v.b = true; p += 4; return v; }
    if (end - p >= 5 && !strncmp(p, "false", 5)) { v.kind = Json::Bool; p += 5; return v; }
    if (end - p >= 4 && !strncmp(p, "null", 4)) { p += 4; return v; }
    char* after = nullptr;
    const std::string text(p, (size_t)(end - p) < 64 ? (size_t)(end - p) : 64);
    v.num = strtod(text.c_str(), &after);
    if (after == text.c_str()) die("weight file header: a value was expected");
    v.kind = Json::Number;
    p += after - text.c_str();
    return v;
  }
};

static std::vector<char> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die(std::string("cannot open ") + path);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> data((size_t)(n > 0 ? n : 0));
  if (n > 0 && fread(data.data(), 1, (size_t)n, f) != (size_t)n) die(std::string("cannot read ") + path);
  fclose(f);
  return data;
}

int main(int argc, char** argv) {
  // ---- the optional storage type of the trunk (DL_DTYPE_F32: the fp32 family)
  int32_t half = DL_DTYPE_F32;
  if (argc > 1 && !strcmp(argv[1], "--half")) {
    if (argc < 3) die("--half needs bf16 or f16");
    half = !strcmp(argv[2], "bf16") ? DL_DTYPE_BF16 : !strcmp(argv[2], "f16") ? DL_DTYPE_F16 : DL_DTYPE_F32;
    if (half == DL_DTYPE_F32) die(std::string("--half: bf16 or f16 expected, got ") + argv[2]);
    argc -= 2;
    argv += 2;
  }
  // ---- the optional record layout
  bool records = false;
  dl_record_layout layout = {12, 0, 4, 8, DL_RECORDS_DROP_ZERO | DL_RECORDS_MIN_RANGE, 0.3f};
  if (argc > 1 && !strcmp(argv[1], "--records")) {
    if (argc < 6) die("--records needs <point_step> <off_x> <off_y> <off_z>");
    int32_t* field[4] = {&layout.point_step, &layout.off_x, &layout.off_y, &layout.off_z};
    for (int k = 0; k < 4; ++k) {
      char* after = nullptr;
      const long v = strtol(argv[2 + k], &after, 10);
      if (after == argv[2 + k] || *after || v < -(1 << 20) || v > (1 << 20)) die(std::string("--records: not a number: ") + argv[2 + k]);
      *field[k] = (int32_t)v;
    }
    if (layout.point_step < 1) die("--records: point_step must be positive");
    records = true;
    argc -= 5;
    argv += 5;
  }
  // ---- the optional pose quality
  bool quality = false;
  int32_t half_rows = 0, half_cols = 0, min_neighbors = 0;
  float epsilon_range = 0.f;
  if (argc > 1 && !strcmp(argv[1], "--quality")) {
    if (argc < 6) die("--quality needs <half_rows> <half_cols> <epsilon_range> <min_neighbors>");
    char* after[4] = {nullptr, nullptr, nullptr, nullptr};
    half_rows = (int32_t)strtol(argv[2], &after[0], 10);
    half_cols = (int32_t)strtol(argv[3], &after[1], 10);
    epsilon_range = strtof(argv[4], &after[2]);
    min_neighbors = (int32_t)strtol(argv[5], &after[3], 10);
    for (int k = 0; k < 4; ++k)
      if (after[k] == argv[2 + k] || *after[k]) die(std::string("--quality: not a number: ") + argv[2 + k]);
    quality = true;
    argc -= 5;
    argv += 5;
  }
  if (argc < 5)
    die("usage: odometry_demo [--half bf16|f16] [--records <point_step> <off_x> <off_y> <off_z>] [--quality <half_rows> <half_cols> <epsilon_range> "
        "<min_neighbors>] <weights.dlpose> <out.txt> <scan0.bin> <scan1.bin> ...   (scans: float32 [3][N], or raw records with --records)");
  const size_t unit = records ? (size_t)layout.point_step : 12;        // bytes per point in a scan file
  // ---- the weight file
  const std::vector<char> blob = read_file(argv[1]);
  if (blob.size() < 16 || memcmp(blob.data(), "DLPOSNET", 8)) die("the weight file has a wrong magic");
  uint32_t version, header_len;
  memcpy(&version, blob.data() + 8, 4);
  memcpy(&header_len, blob.data() + 12, 4);
  if (version != 1) die("the weight file has format version " + std::to_string(version) + ", this program reads 1");
  if (blob.size() < 16 + (size_t)header_len) die("the weight file is truncated inside its header");
  JsonReader reader{blob.data() + 16, blob.data() + 16 + header_len};
  const Json header = reader.value();
  const size_t data_offset = (size_t)header.at("data_offset").integer(), data_bytes = (size_t)header.at("data_bytes").integer();
  if (data_offset < 16 + (size_t)header_len || blob.size() < data_offset + data_bytes) die("the weight file is truncated");
  if (header.at("sensor").kind != Json::Object) die("the weight file names no sensor");
  const Json& sj = header.at("sensor");
  dl_sensor sensor;
  sensor.H = (int32_t)sj.at("H").integer(); sensor.W = (int32_t)sj.at("W").integer();
  sensor.hfov0 = sj.at("hfov").at(0).num; sensor.hfov1 = sj.at("hfov").at(1).num;
  sensor.vfov0 = sj.at("vfov").at(0).num; sensor.vfov1 = sj.at("vfov").at(1).num;
  if (sensor.H < 2 || sensor.W < 2 || sensor.H > (1 << 14) || sensor.W > (1 << 16)) die("the weight file's sensor has an implausible size");
  const int H = sensor.H, W = sensor.W;

  // one device buffer for the whole data section: the arrays keep their 256-byte aligned offsets
  char* d_weights = nullptr;
  HIP_OK(hipMalloc((void**)&d_weights, data_bytes ? data_bytes : 256));
  HIP_OK(hipMemcpy(d_weights, blob.data() + data_offset, data_bytes, hipMemcpyHostToDevice));
  const Json& arrays = header.at("arrays");
  auto address = [&](const std::string& name, size_t floats) -> const float* {
    const Json& e = arrays.at(name);
    const size_t off = (size_t)e.at("offset").integer();
    size_t count = 1;
    for (const Json& d : e.at("shape").items) count *= (size_t)d.integer();
    if (count != floats) die("array " + name + " has " + std::to_string(count) + " elements, the header's sizes ask for " + std::to_string(floats));
    if (off % 256 || off + 4 * count > data_bytes) die("array " + name + " lies outside the data section");
    return (const float*)(d_weights + off);
  };
  // (the struct is large: it lives on the heap)
  std::unique_ptr<dl_pose_net> net_holder(new dl_pose_net);
  dl_pose_net& net = *net_holder;
  memset(&net, 0, sizeof(net));
  const std::string act = header.at("activation").str;
  net.act = act == "relu" ? DL_POSE_ACT_RELU : act == "tanh" ? DL_POSE_ACT_TANH : 0;
  const Json& blocks = header.at("blocks");
  if (blocks.kind != Json::Array || blocks.items.empty() || blocks.items.size() > DL_POSE_NET_MAX_BLOCKS) die("the weight file has a bad number of blocks");
  net.n_blocks = (int32_t)blocks.items.size();
  net.F = (int32_t)header.at("F").integer(); net.R = (int32_t)header.at("R").integer(); net.Hd = (int32_t)header.at("Hd").integer();
  if (net.F < 1 || net.R < 1 || net.Hd < 1) die("the weight file has bad head sizes");
  net.conv1_w = address("conv1_w", 64 * 3 * 3 * 8);
  for (int i = 0; i < net.n_blocks; ++i) {
    const Json& bj = blocks.at((size_t)i);
    dl_pose_block& b = net.blocks[i];
    b.cin = (int32_t)bj.at("cin").integer(); b.cout = (int32_t)bj.at("cout").integer();
    b.stride_h = (int32_t)bj.at("stride").at(0).integer(); b.stride_w = (int32_t)bj.at("stride").at(1).integer();
    b.has_downsample = bj.at("has_downsample").b ? 1 : 0;
    if (b.cin < 1 || b.cout < 1 || b.cin > (1 << 14) || b.cout > (1 << 14)) die("the weight file has bad channel counts");
    const std::string base = "blocks." + std::to_string(i) + ".";
    b.w1 = address(base + "w1", (size_t)b.cout * 9 * b.cin);
    b.w2 = address(base + "w2", (size_t)b.cout * 9 * b.cout);
    b.wd = b.has_downsample ? address(base + "wd", (size_t)b.cout * b.cin) : nullptr;
  }
  const size_t F = (size_t)net.F, R = (size_t)net.R, Hd = (size_t)net.Hd;
  net.heads.fc_w = address("heads.fc_w", R * F); net.heads.fc_b = address("heads.fc_b", R);
  net.heads.r1_w = address("heads.r1_w", Hd * R); net.heads.r1_b = address("heads.r1_b", Hd);
  net.heads.r3_w = address("heads.r3_w", 4 * Hd); net.heads.r3_b = address("heads.r3_b", 4);
  net.heads.t1_w = address("heads.t1_w", Hd * R); net.heads.t1_b = address("heads.t1_b", Hd);
  net.heads.t3_w = address("heads.t3_w", 3 * Hd); net.heads.t3_b = address("heads.t3_b", 3);

  // ---- the scans (read first: the largest one sizes the workspace)
  std::vector<std::vector<char>> scans;
  size_t max_points = 0;
  for (int i = 3; i < argc; ++i) {
    scans.push_back(read_file(argv[i]));
    if (scans.back().size() % unit) die(std::string(argv[i]) + (records ? " does not hold whole records" : " is not a float32 [3][N] file"));
    if (scans.back().size() / unit > ((size_t)1 << 30)) die(std::string(argv[i]) + " is too large");
    if (scans.back().size() / unit > max_points) max_points = scans.back().size() / unit;
  }

  // ---- buffers: all owned here, the library allocates nothing
  const size_t prepared_bytes = half ? dl_pose_net_prepared_bytes_h(&net, 1, H, W, half) : dl_pose_net_prepared_bytes(&net, 1, H, W);
  if (!prepared_bytes) die(std::string("dl_pose_net_prepared_bytes: ") + dl_last_error());
  // (the records path keeps no staging records: its workspace does not grow with the scan)
  const size_t ws_bytes = half ? dl_odometry_workspace_bytes_h(&net, &sensor, records ? 0 : (int32_t)max_points, H, W, half)
                               : dl_odometry_workspace_bytes(&net, &sensor, records ? 0 : (int32_t)max_points, H, W);
  if (!ws_bytes) die(std::string("dl_odometry_workspace_bytes: ") + dl_last_error());
  void *prepared = nullptr, *workspace = nullptr;
  float *images[2] = {nullptr, nullptr}, *d_pts = nullptr, *d_out = nullptr;
  int32_t* d_offs = nullptr;
  HIP_OK(hipMalloc(&prepared, prepared_bytes));
  HIP_OK(hipMalloc(&workspace, ws_bytes));
  HIP_OK(hipMalloc((void**)&images[0], (size_t)4 * H * W * 4));
  HIP_OK(hipMalloc((void**)&images[1], (size_t)4 * H * W * 4));
  HIP_OK(hipMalloc((void**)&d_pts, max_points ? max_points * unit : 256));
  HIP_OK(hipMalloc((void**)&d_offs, 256));
  HIP_OK(hipMalloc((void**)&d_out, 256));                              // translation [3] | quaternion [4] | T [16] at floats 0, 4, 8
  // pose quality: one dl_scan_geometry record beside each image, the call's workspace and its outputs (doubles 0.. info [36] | rhs [6] |
  // stats [2] | covariance [36], then the int32 status)
  dl_scan_geometry records_geometry[2] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  void* quality_ws = nullptr;
  double* d_quality = nullptr;
  if (quality) {
    const size_t q_bytes = dl_odometry_quality_workspace_bytes(&sensor, H, W);
    if (!q_bytes) die(std::string("dl_odometry_quality_workspace_bytes: ") + dl_last_error());
    HIP_OK(hipMalloc(&quality_ws, q_bytes));
    HIP_OK(hipMalloc((void**)&d_quality, 81 * sizeof(double)));
    for (int k = 0; k < 2; ++k) {
      HIP_OK(hipMalloc((void**)&records_geometry[k].normals, (size_t)3 * H * W * 4));
      HIP_OK(hipMalloc((void**)&records_geometry[k].packed_image, (size_t)4 * H * W * 4));
      HIP_OK(hipMalloc((void**)&records_geometry[k].packed_normals, (size_t)4 * H * W * 4));
    }
  }
  hipStream_t stream;
  HIP_OK(hipStreamCreate(&stream));
  if (half) DL_OK_OR_DIE(dl_pose_net_prepare_h(&net, 1, H, W, half, prepared, stream));
  else DL_OK_OR_DIE(dl_pose_net_prepare(&net, 1, H, W, prepared, stream));

  FILE* out = fopen(argv[2], "w");
  if (!out) die(std::string("cannot write ") + argv[2]);
  double pose[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  int cur = 0;
  for (size_t i = 0; i < scans.size(); ++i) {
    const size_t n = scans[i].size() / unit;
    if (n) HIP_OK(hipMemcpyAsync(d_pts, scans[i].data(), n * unit, hipMemcpyHostToDevice, stream));
    if (i) cur = 1 - cur;                                            // the caller's swap of the two image buffers
    const float* prev = i ? images[1 - cur] : nullptr;
    if (records && half)
      DL_OK_OR_DIE(dl_odometry_push_records_h(&net, prepared, &sensor, d_pts, (int32_t)n, &layout, d_offs, prev, images[cur], half, workspace, d_out,
                                              d_out + 4, d_out + 8, stream));
    else if (half)
      DL_OK_OR_DIE(dl_odometry_push_h(&net, prepared, &sensor, d_pts, (int64_t)n, (int32_t)n, d_offs, prev, images[cur], half, workspace, d_out, d_out + 4,
                                      d_out + 8, stream));
    else if (records)
      DL_OK_OR_DIE(dl_odometry_push_records(&net, prepared, &sensor, d_pts, (int32_t)n, &layout, d_offs, i ? images[1 - cur] : nullptr, images[cur],
                                            workspace, d_out, d_out + 4, d_out + 8, stream));
    else
      DL_OK_OR_DIE(dl_odometry_push(&net, prepared, &sensor, d_pts, (int64_t)n, (int32_t)n, d_offs, i ? images[1 - cur] : nullptr, images[cur], workspace,
                                    d_out, d_out + 4, d_out + 8, stream));
    if (quality)                                                     // the records swap with the images
      DL_OK_OR_DIE(dl_odometry_quality(&sensor, prev, i ? &records_geometry[1 - cur] : nullptr, images[cur], &records_geometry[cur], d_out + 8, half_rows,
                                       half_cols, epsilon_range, min_neighbors, quality_ws, d_quality, d_quality + 36, d_quality + 42, d_quality + 44,
                                       (int32_t*)(d_quality + 80), stream));
    float T[16];
    double q_host[81];
    if (i) HIP_OK(hipMemcpyAsync(T, d_out + 8, sizeof(T), hipMemcpyDeviceToHost, stream));
    if (i && quality) HIP_OK(hipMemcpyAsync(q_host, d_quality, sizeof(q_host), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));                            // (also: the scan buffer is free for the next copy)
    if (!i) continue;
    double next[4][4];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += pose[r][k] * (double)T[4 * k + c];
        next[r][c] = s;
      }
    memcpy(pose, next, sizeof(pose));
    fprintf(out, "%zu T", i);
    for (int k = 0; k < 16; ++k) {
      uint32_t bits;
      memcpy(&bits, &T[k], 4);
      fprintf(out, " %08x", bits);
    }
    fprintf(out, " pose");
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) fprintf(out, " %.9e", pose[r][c]);
    if (quality) {
      int32_t status;
      memcpy(&status, &q_host[80], 4);
      fprintf(out, " quality %d pairs %.0f cov_diag", status, q_host[43]);
      printf("push %zu: status %d, %.0f pairs, covariance diagonal", i, status, q_host[43]);
      for (int k = 0; k < 6; ++k) {
        fprintf(out, " %.9e", q_host[44 + 7 * k]);
        printf(" %.3e", q_host[44 + 7 * k]);
      }
      printf("\n");
    }
    fprintf(out, "\n");
  }
  if (fclose(out)) die(std::string("cannot finish ") + argv[2]);
  HIP_OK(hipStreamDestroy(stream));
  for (void* p : {(void*)d_weights, prepared, workspace, (void*)images[0], (void*)images[1], (void*)d_pts, (void*)d_offs, (void*)d_out, quality_ws,
                  (void*)d_quality, (void*)records_geometry[0].normals, (void*)records_geometry[0].packed_image, (void*)records_geometry[0].packed_normals,
                  (void*)records_geometry[1].normals, (void*)records_geometry[1].packed_image, (void*)records_geometry[1].packed_normals})
    if (p) HIP_OK(hipFree(p));
  printf("odometry_demo: %zu scans, %zu poses -> %s\n", scans.size(), scans.empty() ? (size_t)0 : scans.size() - 1, argv[2]);
  return 0;
}
