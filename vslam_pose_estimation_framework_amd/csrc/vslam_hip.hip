// vslam_hip.hip — the one translation unit of libvslam_hip.so: the kernels, then the host side behind the C ABI of include/vslam_hip.h in
// dependency order.  gfx950 only; there is no CPU fallback: every entry point fails with VSLAM_ERR_NO_DEVICE / VSLAM_ERR_HIP when the
// GPU path is unusable.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kernels_stage.h"     // -> kernels_frame2.h -> kernels_stereo.h -> kernels_recover.h -> kernels_frame.h
#include "kernels_motion.h"    // the frame's motion prior under VSLAM_MOTION_NONE / CAMERA_ODOMETRY
#include "kernels_depth.h"
#include "kernels_orb.h"
#include "kernels_landmark.h"
#include "kernels_report.h"
#include "kernels_rectify.h"
#include "kernels_undistort.h"
#include "kernels_equalize.h"
#include "kernels_clahe.h"
#include "kernels_bilateral.h"
#include "kernels_gray.h"
#include "kernels_downscale.h" // integer-factor reduction of images and depth images (stand-alone entries)
#include "kernels_smooth.h"    // Gaussian / median smoothing of the intensity image
#include "kernels_map.h"
#include "kernels_obs.h"
#include "kernels_map_color.h"
#include "kernels_mask.h"      // detection masks: pack + erode, apply between k_fast_box and k_emit

#define VS_API extern "C" __attribute__((visibility("default")))

#include "device_store.h"    // memory a switchable feature owns on the device
#include "stage_plan.h"      // the stereo context's input stages as a plan: which slabs exist, a frame's route (plain C++)
#include "host_prestage.h"   // the input stages (grey, remap, equalisation slot) as the stereo context and the RGB-D tracker share them
#include "host_ctx.h"        // the context: allocation, scratch, timers, configuration, create / destroy / reset, stream lifetime
#include "host_switches.h"   // the context's input-stage switches and their getters: rectification, equalisation / CLAHE, colour input
#include "host_frame.h"      // a frame's inputs, its routing through the input stages and its two launch sequences
#include "host_readback.h"   // vslam_get_*: frame results, the landmark map, the observation log, poses, timers
#include "host_entries.h"    // stand-alone component entries (one piece of the pipeline on caller data)
#include "host_stage.h"      // stage entries (the reference's plug-in virtuals), stage reports and their views
#include "host_rgbd.h"       // vslam_rgbd_*: RGB-D mode
#include "host_comm.h"       // pose all-gather on RCCL
