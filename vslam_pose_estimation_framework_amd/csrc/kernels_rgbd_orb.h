// kernels_rgbd_orb.h — detector_type ORB inside the device-resident RGB-D loop (rgbd_device.h enqueue_orb_detect).  gfx950, wave64.
//
// An OrbDetector (base_framepoint_generator.cpp:52-70) is cv::ORB::create(5000, 1.2, 8, 31, 0, 2, HARRIS_SCORE, 31, threshold)->detect on every
// detector region's VIEW of the image, then the configured extractor on the whole image.  vslam_orb_detect / vslam_orb_describe_keypoints
// (host_entries.h) are the stand-alone statement of it, one region and one sequence per call with host arithmetic in between; here the same
// steps run for all sequences, regions and pyramid levels of a batch on the frame's queue, and nothing is read back:
//
//   k_orbd_begin            level 0 of every region's pyramid (the region's view of the prestaged image); the regions' FAST thresholds
//                           into the level contexts
//   k_orbd_resize           level l from level l - 1 (k_resize_linear_u8's arithmetic, resize_linear_px), per level
//   k_fast_box, k_emit      unchanged, on a level-sized DevCfg / DevBuf pair per level whose streams are the (sequence, region) pairs:
//                           FAST-9/16, strict NMS, runByImageBorder(31), row-major corners with 8-bit scores
//   k_orbd_select_fast      retainBest(2 n) on the FAST score        } one workgroup / wavefront set per (sequence, region, level):
//   k_orbd_harris           HarrisResponses                          } orb_select_body, orb_harris_one, orb_angle_one of kernels_orb.h
//   k_orbd_select_harris    retainBest(n) on the Harris response     }
//   k_orbd_control          per sequence: where each (region, level) list lands in the keypoint vector (region-major, level-major), the
//                           regions' threshold controllers on their own counts (k_emit's run_controller == 2 arithmetic), capacity
//   k_orbd_angle            ICAngles; the keypoint scaled back to level 0 and shifted by the region's corner (two float operations)
//   k_orbd_gauss7, k_orbd_describe | k_orbd_brief      ORB::compute on the keypoint's own level and angle | BRIEF at level 0
//   k_orbd_install          the extractor's keep filter, the union with the frame's earlier attempts, cv::ORB::compute's level-major
//                           regroup, and the feature store the tracker reads: arrays sorted by lattice pixel, row / cell CSR, order, fvis
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_rgbd.h"
#include "kernels_orb.h"
#include "orb_plan.h"

#define VS_ORBD_LEVELS 8      // cv::ORB::create(.., nlevels = 8, ..)
#define VS_ORBD_FEATURES 5000
#define VS_ORBD_EDGE 31
#define VS_ORBD_PATCH 31

struct OrbdLevel {
  int32_t rows, cols, stride, quota, nmax;   // a region's view at this level; capacity of the level's corner list
  float sc;                                  // (float)pow(1.2, level)
  uint8_t* pyr;                              // [B * R][rows * stride]
  // what k_emit leaves in the level context (slices of stream z at 2 * z: DevBuf keeps two image sides per stream)
  const int16_t* kp_xy; const uint8_t* kp_score; const int32_t* n_kp; StreamState* st;
  int16_t* xy1; int16_t* xy2; float* r1; float* rh; float* r2; int32_t* n1; int32_t* n2;     // [B * R][nmax] / [B * R]
  // the whole image at this level (the extractor's pyramid): its 7 x 7 Gaussian [B][wrows * wstride]; level 0's is the inner context's
  int32_t wrows, wcols, wstride;
  const uint8_t* wblur;
};
struct OrbDet {
  int32_t L, R, B, NMAX;
  int32_t rx[VSLAM_MAX_REGIONS], ry[VSLAM_MAX_REGIONS];
  OrbdLevel lv[VS_ORBD_LEVELS];
  OrbUmax um;
  int32_t* base;      // [B][R * L + 1] first vector position of every (region, level) list
  int32_t* n_new;     // [B] keypoints of this detection (clipped to NMAX)
  float* kp;          // [B][NMAX][4] x, y, angle, level
  uint8_t* keep;      // [B][NMAX]
  uint8_t* kdesc;     // [B][NMAX][32]
  // the frame's keypoint vector in vector order while k_orbd_install rebuilds the store
  uint32_t* v_key; int32_t* v_vp; uint8_t* v_lvl; float* v_fxy; uint8_t* v_desc; uint32_t* s_key;     // [B][NMAX] each
  int32_t* bucket;                           // [B][NMAX] vector elements grouped by image row (any order inside a row)
  int32_t* row_start; int32_t* row_fill;     // [B][rows + 1]
};

__global__ __launch_bounds__(256) void k_orbd_begin(const DevCfg c, const DevBuf b, const OrbDet* od) {
  const int z = blockIdx.z, R = od->R, s = z / R, r = z - s * R;
  if (!vs_active(b, s)) return;
  const OrbdLevel& l0 = od->lv[0];
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x < l0.cols && y < l0.rows) {
    const uint8_t* img = b.img[0] + (size_t)s * b.img_stream_stride + (size_t)(od->ry[r] + y) * b.img_row_stride + od->rx[r];
    l0.pyr[((size_t)z * l0.rows + y) * l0.stride + x] = img[x];
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < od->L) {
    StreamState& ls = od->lv[threadIdx.x].st[z];
    ls.thr[0] = b.st[s].thr[r];
    ls.error_flags = 0;
  }
}
// grid z = images; the activity bit of image z is that of sequence z / per_seq
__global__ __launch_bounds__(256) void k_orbd_resize(const DevBuf act, int per_seq, const uint8_t* src, int rows, int cols, int stride, size_t sstream,
                                                     uint8_t* dst, int drows, int dcols, int dstride, size_t dstream) {
  const int z = blockIdx.z;
  if (!vs_active(act, z / per_seq)) return;
  const int dx = blockIdx.x * 256 + threadIdx.x, dy = blockIdx.y;
  if (dx >= dcols || dy >= drows) return;
  dst[(size_t)z * dstream + (size_t)dy * dstride + dx] = resize_linear_px(src + (size_t)z * sstream, rows, cols, stride, dx, dy, drows, dcols);
}
__global__ __launch_bounds__(256) void k_orbd_gauss7(const DevBuf act, const uint8_t* img, int stride, int rows, int cols, size_t sstream, const Gauss7 g,
                                                     uint8_t* out, int ostride, size_t ostream) {
  __shared__ uint8_t src[VS_TILE_H + 6][72];
  __shared__ uint16_t hs[VS_TILE_H + 6][VS_TILE_W];
  const int z = blockIdx.z;
  if (!vs_active(act, z)) return;
  gauss7_tile(img + (size_t)z * sstream, stride, rows, cols, blockIdx.x * VS_TILE_W, blockIdx.y * VS_TILE_H, g, out + (size_t)z * ostream, ostride, src, hs);
}

// grid (B * R, L)
__global__ __launch_bounds__(1024) void k_orbd_select_fast(const DevBuf act, const OrbDet* od) {
  const int z = blockIdx.x;
  if (!vs_active(act, z / od->R)) return;
  const OrbdLevel& v = od->lv[blockIdx.y];
  const size_t o = (size_t)z * v.nmax;
  orb_select_body<uint8_t>(v.n_kp[2 * z], v.kp_xy + 2 * o * 2, v.kp_score + 2 * o, 2 * v.quota, v.n1 + z, v.xy1 + o * 2, v.r1 + o, v.nmax);
}
__global__ __launch_bounds__(1024) void k_orbd_select_harris(const DevBuf act, const OrbDet* od) {
  const int z = blockIdx.x;
  if (!vs_active(act, z / od->R)) return;
  const OrbdLevel& v = od->lv[blockIdx.y];
  const size_t o = (size_t)z * v.nmax;
  orb_select_body<float>(v.n1[z], v.xy1 + o * 2, v.rh + o, v.quota, v.n2 + z, v.xy2 + o * 2, v.r2 + o, v.nmax);
}
// grid (x, B * R, L): one wavefront per keypoint.  Corners lie 31 px inside the level image: the 9 x 9 window is inside it
__global__ __launch_bounds__(256) void k_orbd_harris(const DevBuf act, const OrbDet* od) {
  const int z = blockIdx.y;
  if (!vs_active(act, z / od->R)) return;
  const OrbdLevel& v = od->lv[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const size_t o = (size_t)z * v.nmax;
  const uint8_t* img = v.pyr + (size_t)z * v.rows * v.stride;
  const int16_t* xy = v.xy1 + o * 2;
  const int n = v.n1[z];
  for (int i = wave; i < n; i += nwaves) {
    const float h = orb_harris_one(img, v.stride, xy[2 * i], xy[2 * i + 1], lane);
    if (lane == 0) v.rh[o + i] = h;
  }
}
// one workgroup per sequence; the work is R * L additions and R controllers
__global__ __launch_bounds__(64) void k_orbd_control(const DevCfg c, const DevBuf b, const OrbDet* od) {
  const int s = blockIdx.x;
  if (!vs_active(b, s) || threadIdx.x != 0) return;
  const int R = od->R, L = od->L;
  StreamState& st = b.st[s];
  int32_t* base = od->base + (size_t)s * (R * L + 1);
  const double tol = c.c.target_number_of_keypoints_tolerance, maxchg = c.c.detector_threshold_maximum_change;
  const double tmin = c.c.detector_threshold_minimum, tmax = c.c.detector_threshold_maximum;
  const double target = (double)c.target_per_detector;
  int total = 0;
  bool over = false;
  for (int r = 0; r < R; ++r) {
    const int z = s * R + r;
    int nr = 0;
    for (int l = 0; l < L; ++l) {
      const OrbdLevel& v = od->lv[l];
      base[r * L + l] = total;
      const int n2 = v.n2[z];
      total += n2; nr += n2;
      over = over || (v.st[z].error_flags & 1) || (v.nmax == 65535 && v.n_kp[2 * z] >= 65535);     // more than 65535 FAST corners on a level
    }
    b.iinfo[s].raw_count[0][r] = nr;
    // detectKeypoints' controller on the region's own count (base_framepoint_generator.cpp:382-415), adjustDetectorThresholds over one detection
    double t = (double)st.thr[r];
    const double delta = ((double)nr - target) / target;
    if (delta < -tol) {
      const double change = fmax(delta, -maxchg);
      t = t + fmin(change * t, -1.0);
      if (t < tmin) t = tmin;
    } else if (delta > tol) {
      const double change = fmin(delta, maxchg);
      t += fmax(change * t, 1.0);
      if (t > tmax) t = tmax;
    }
    st.thr[r] = (int)rint(t / 1);
  }
  base[R * L] = total;
  for (int r = 0; r < R; ++r) b.iinfo[s].thr_after[r] = st.thr[r];
  if (over || total > od->NMAX) atomicOr(&st.error_flags, 1);          // the frame fails with VSLAM_ERR_CAPACITY, as after k_emit's overflow
  od->n_new[s] = min(total, od->NMAX);
}
// grid (x, B * R, L): the patch (radius 15) is inside the level image for the same reason as the Harris window
__global__ __launch_bounds__(256) void k_orbd_angle(const DevBuf act, const OrbDet* od) {
  const int z = blockIdx.y, R = od->R, s = z / R, r = z - s * R, l = blockIdx.z;
  if (!vs_active(act, s)) return;
  const OrbdLevel& v = od->lv[l];
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const size_t o = (size_t)z * v.nmax;
  const uint8_t* img = v.pyr + (size_t)z * v.rows * v.stride;
  const int16_t* xy = v.xy2 + o * 2;
  const int n = v.n2[z];
  const int at0 = od->base[(size_t)s * (R * od->L + 1) + r * od->L + l];
  const float cx = (float)od->rx[r], cy = (float)od->ry[r];
  for (int i = wave; i < n; i += nwaves) {
    const int x0 = xy[2 * i], y0 = xy[2 * i + 1];
    const float ang = orb_angle_one(img, v.stride, x0, y0, VS_ORBD_PATCH / 2, od->um, lane);
    if (lane == 0 && at0 + i < od->NMAX) {
      float* kp = od->kp + ((size_t)s * od->NMAX + at0 + i) * 4;
      const float fx = l ? (float)x0 * v.sc : (float)x0, fy = l ? (float)y0 * v.sc : (float)y0;      // the detector's scale-back ...
      kp[0] = fx + cx; kp[1] = fy + cy; kp[2] = ang; kp[3] = (float)l;                                // ... then keypoint.pt += region corner
    }
  }
}

// ORB::compute on the detection (vslam_orb_describe_keypoints' host arithmetic restated): position at the keypoint's level lrint(pt * (1 / scale)),
// runByImageBorder(31) at level 0 and the pattern's reach at the level, the rotation as OpenCV evaluates it — the angle in float radians,
// cos / sin in double, rounded to float.  grid (x, B), one wavefront per keypoint.
__global__ __launch_bounds__(256) void k_orbd_describe(const DevCfg c, const DevBuf b, const OrbDet* od) {
  const int s = blockIdx.y;
  if (!vs_active(b, s)) return;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const int n = od->n_new[s], rows = c.c.rows, cols = c.c.cols;
  const int reach = 23;
  for (int i = wave; i < n; i += nwaves) {
    const float* kp = od->kp + ((size_t)s * od->NMAX + i) * 4;
    const int lv = (int)kp[3];
    const OrbdLevel& v = od->lv[lv];
    const float inv = 1.f / v.sc;
    const int px = (int)rintf(kp[0] * inv), py = (int)rintf(kp[1] * inv);
    const int x0 = (int)rintf(kp[0]), y0 = (int)rintf(kp[1]);
    const int lrows = lv ? v.wrows : rows, lcols = lv ? v.wcols : cols, stride = lv ? v.wstride : c.bstride;
    const bool in = x0 >= VSLAM_ORB_BORDER && x0 < cols - VSLAM_ORB_BORDER && y0 >= VSLAM_ORB_BORDER && y0 < rows - VSLAM_ORB_BORDER &&
                    px >= reach && py >= reach && px < lcols - reach && py < lrows - reach;
    unsigned long long d[4] = {0ull, 0ull, 0ull, 0ull};
    if (in) {
      float angle = kp[2];
      angle *= (float)(3.1415926535897932384626433832795 / 180.f);
      const float a = (float)cos((double)angle), bs = (float)sin((double)angle);
      const uint8_t* blur = lv ? v.wblur + (size_t)s * v.wrows * v.wstride : blur_of(c, b, s, 0);
      const OrbTaps t = orb_taps(lane, a, bs, stride);
      orb_wave(blur + (size_t)py * stride + px, t, d);
    }
    if (lane == 0) od->keep[(size_t)s * od->NMAX + i] = in ? 1 : 0;
    const unsigned long long dv = lane == 0 ? d[0] : (lane == 1 ? d[1] : (lane == 2 ? d[2] : d[3]));
    if (lane < 4) reinterpret_cast<unsigned long long*>(od->kdesc + ((size_t)s * od->NMAX + i) * 32)[lane] = dv;
  }
}
// BriefDescriptorExtractor: level 0, pixel (int)(pt + 0.5), on the whole frame's box image
__global__ __launch_bounds__(256) void k_orbd_brief(const DevCfg c, const DevBuf b, const OrbDet* od) {
  const int s = blockIdx.y;
  if (!vs_active(b, s)) return;
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const int n = od->n_new[s], rows = c.c.rows, cols = c.c.cols;
  const uint16_t* box = box_of(c, b, s, 0);
  for (int i = wave; i < n; i += nwaves) {
    const float* kp = od->kp + ((size_t)s * od->NMAX + i) * 4;
    const int x = (int16_t)(int)(kp[0] + 0.5f), y = (int16_t)(int)(kp[1] + 0.5f);
    const bool in = x >= VSLAM_BRIEF_BORDER && x < cols - VSLAM_BRIEF_BORDER && y >= VSLAM_BRIEF_BORDER && y < rows - VSLAM_BRIEF_BORDER;
    uint8_t* out = od->kdesc + ((size_t)s * od->NMAX + i) * 32;
    if (lane == 0) od->keep[(size_t)s * od->NMAX + i] = in ? 1 : 0;
    if (in) brief_wave(box, c.bstride, x, y, lane, out);
    else if (lane < 4) reinterpret_cast<unsigned long long*>(out)[lane] = 0ull;
  }
}

// The feature store of one initialize() (one workgroup per sequence).  The frame's keypoint vector is [the earlier attempts' keypoints in their
// order (again), this detection's kept keypoints in detection order]; cv::ORB::compute regroups a vector that is not level-sorted level-major,
// stable, and the regrouped order is the vector's from then on (rgbd_tracker.h initialize(), tests/rgbd_loop.py).  The store is rebuilt from
// the vector: arrays sorted by lattice pixel with equal pixels in vector order, the row / cell CSR, order[vector position] = sorted index and
// fvis = the lattice's last writer in vector order (orb_plan.h has the arithmetic; an element is ranked among the elements of its own image row).
__global__ __launch_bounds__(1024) void k_orbd_install(const DevCfg c, const DevBuf b, const RgbdBuf all, const OrbDet* od, int again) {
  __shared__ int sh[17];
  __shared__ int unsorted;
  const int sq = blockIdx.x;
  if (!vs_active(b, sq)) return;
  const RgbdBuf r = rgbd_stream(all, sq);
  RgbdState& st = *r.st;
  if (again && st.done) return;
  const int tid = threadIdx.x, NT = blockDim.x, N = c.NMAX;
  const size_t o = (size_t)sq * N;
  uint32_t* v_key = od->v_key + o; int32_t* v_vp = od->v_vp + o; uint8_t* v_lvl = od->v_lvl + o; float* v_fxy = od->v_fxy + o * 2;
  uint8_t* v_desc = od->v_desc + o * 32; uint32_t* s_key = od->s_key + o;
  int16_t* kxy = kpxy_of(c, b, sq, 0);
  uint8_t* desc = desc_of(c, b, sq, 0);
  uint8_t* ksc = kpscore_of(c, b, sq, 0);
  uint8_t* used = used_of(c, b, sq, 0);
  int32_t* rc = rowcell_of(c, b, sq, 0);
  const int nA = again ? min(b.n_kp[2 * sq], N) : 0;
  if (tid == 0) unsorted = 0;
  // the vector so far, out of the store
  for (int v = tid; v < nA; v += NT) {
    const int f = r.order[v];
    v_fxy[2 * v] = r.fkxy[2 * f]; v_fxy[2 * v + 1] = r.fkxy[2 * f + 1]; v_lvl[v] = r.flvl[f];
    rgbd_copy_desc(v_desc + (size_t)32 * v, desc + (size_t)32 * f);
  }
  // this detection behind it: the extractor's keep filter, order kept
  const int nD = od->n_new[sq];
  const float* kp = od->kp + o * 4;
  const uint8_t* keep = od->keep + o;
  const uint8_t* kdesc = od->kdesc + o * 32;
  int n = nA;
  for (int i0 = 0; i0 < nD; i0 += NT) {
    const int i = i0 + tid;
    const int k = (i < nD && keep[i]) ? 1 : 0;
    int total;
    const int at = n + block_exclusive_scan(k, sh, &total);
    if (k && at < N) {
      v_fxy[2 * at] = kp[4 * i]; v_fxy[2 * at + 1] = kp[4 * i + 1]; v_lvl[at] = (uint8_t)(int)kp[4 * i + 3];
      rgbd_copy_desc(v_desc + (size_t)32 * at, kdesc + (size_t)32 * i);
    }
    n += total;
  }
  if (n > N) {                                // the frame fails with VSLAM_ERR_CAPACITY (bit 0, like k_emit's overflow); the store stays as it was
    if (tid == 0) atomicOr(&st.error_flags, 1);
    return;
  }
  __syncthreads();
  for (int v = tid; v < n; v += NT) {
    v_key[v] = orbd_pixel_key(v_fxy[2 * v], v_fxy[2 * v + 1]);
    if (v > 0 && v_lvl[v] < v_lvl[v - 1]) unsorted = 1;
  }
  __syncthreads();
  const bool regroup = r.p.descriptor_type == VSLAM_DESCRIPTOR_ORB && unsorted != 0;
  if (regroup) {
    // orbd_regroup_pos for every element at once: per level, a running count over the vector (elements of lower levels in front)
    int placed = 0;
    for (int l = 0; l < od->L; ++l)
      for (int v0 = 0; v0 < n; v0 += NT) {
        const int v = v0 + tid;
        const int f = (v < n && v_lvl[v] == l) ? 1 : 0;
        int total;
        const int at = placed + block_exclusive_scan(f, sh, &total);
        if (f) v_vp[v] = at;
        placed += total;
      }
  } else {
    for (int v = tid; v < n; v += NT) v_vp[v] = v;
  }
  // the vector's elements grouped by image row: counts, starts, members (a row holds a few dozen at most on camera images)
  const int rows = c.c.rows;
  int32_t* row_start = od->row_start + (size_t)sq * (rows + 1);
  int32_t* row_fill = od->row_fill + (size_t)sq * (rows + 1);
  int32_t* bucket = od->bucket + o;
  for (int y = tid; y <= rows; y += NT) row_fill[y] = 0;
  __syncthreads();
  for (int v = tid; v < n; v += NT) atomicAdd(&row_fill[min((int)(v_key[v] >> 16), rows - 1)], 1);
  __syncthreads();
  {
    int run = 0;
    for (int y0 = 0; y0 < rows; y0 += NT) {
      const int y = y0 + tid;
      const int cnt = y < rows ? row_fill[y] : 0;
      int total;
      const int at = run + block_exclusive_scan(cnt, sh, &total);
      if (y < rows) row_start[y] = at;
      run += total;
    }
    if (tid == 0) row_start[rows] = run;
  }
  __syncthreads();
  for (int y = tid; y < rows; y += NT) row_fill[y] = 0;
  __syncthreads();
  for (int v = tid; v < n; v += NT) {
    const int y = min((int)(v_key[v] >> 16), rows - 1);
    bucket[row_start[y] + atomicAdd(&row_fill[y], 1)] = v;
  }
  __syncthreads();
  for (int v = tid; v < n; v += NT) {
    bool vis;
    const int yr = min((int)(v_key[v] >> 16), rows - 1);
    const int b0 = row_start[yr];
    const int at = b0 + orbd_rank(v_key, v_vp, bucket + b0, row_start[yr + 1] - b0, v, &vis);
    const float x = v_fxy[2 * v], y = v_fxy[2 * v + 1];
    kxy[2 * at] = (int16_t)(int)x; kxy[2 * at + 1] = (int16_t)(int)y;       // IntensityFeature: row = (int)pt.y, col = (int)pt.x
    r.fkxy[2 * at] = x; r.fkxy[2 * at + 1] = y; r.flvl[at] = v_lvl[v];
    rgbd_copy_desc(desc + (size_t)32 * at, v_desc + (size_t)32 * v);
    ksc[at] = 0; used[at] = 0;
    r.fvis[at] = vis ? 1 : 0;
    r.order[v_vp[v]] = at;
    s_key[at] = v_key[v];
  }
  __syncthreads();
  const int CW1 = c.CW + 1;
  for (int e = tid; e < r.ncsr; e += NT) {
    const int row = e / CW1, cc = e - row * CW1;
    rc[e] = orbd_lower_bound(s_key, n, ((uint32_t)row << 16) | (uint32_t)min(16 * cc, 0xFFFF));
  }
  if (tid == 0) { b.n_kp[2 * sq] = n; st.n_acc = nA; st.merged = 1; }       // merged: order and fvis are the store's own (rgbd_features, rgbd_track_args)
}
