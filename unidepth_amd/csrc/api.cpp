// Error plumbing + library info for the C-ABI (include/unidepth_hip.h).
#include <string.h>
#include "ud_common.h"

static thread_local char g_err[256] = "";

void ud_set_error(const char* msg) {
  strncpy(g_err, msg ? msg : "", sizeof(g_err) - 1);
  g_err[sizeof(g_err) - 1] = 0;
}

extern "C" const char* ud_last_error(void) { return g_err; }
extern "C" int ud_version(void) { return 128; }

// struct sizes, so the Python binding can verify its ctypes mirror of include/unidepth_hip.h
extern "C" int ud_struct_size(int which) {
  switch (which) {
    case 0: return (int)sizeof(UdGemm);
    case 1: return (int)sizeof(UdLayerNorm);
    case 2: return (int)sizeof(UdAttention);
    case 3: return (int)sizeof(UdPreprocess);
    case 4: return (int)sizeof(UdRayEmbed);
    case 5: return (int)sizeof(UdUpsample2x);
    case 6: return (int)sizeof(UdResizeAC);
    case 7: return (int)sizeof(UdFinalize);
    case 8: return (int)sizeof(UdLinearF32);
    case 9: return (int)sizeof(UdDwConv7);
    case 10: return (int)sizeof(UdV1Op);
    case 11: return (int)sizeof(UdKnn);
    case 12: return (int)sizeof(UdExtractPatches);
    case 13: return (int)sizeof(UdCameraHead);
    case 14: return (int)sizeof(UdEvalDepth);
    case 15: return (int)sizeof(UdPointCloud);
    case 17: return (int)sizeof(UdMatchGt);     // 16 stays unassigned (-1)
    case 18: return (int)sizeof(UdColorize);
    case 20: return (int)sizeof(UdSplat);        // 19 stays unassigned (-1)
    case 21: return (int)sizeof(UdDepthMinPool);
    case 23: return (int)sizeof(UdResizeAA);     // 22 stays unassigned (-1)
    case 25: return (int)sizeof(UdEval3d);       // 24 stays unassigned (-1)
    case 27: return (int)sizeof(UdReconstruct);  // 26 stays unassigned (-1)
    case 28: return (int)sizeof(UdCameraProject);
    case 29: return (int)sizeof(UdSplatCamera);
    case 31: return (int)sizeof(UdCameraUnproject);  // 30 stays unassigned (-1)
    case 33: return (int)sizeof(UdRemap);            // 32 stays unassigned (-1)
    case 34: return (int)sizeof(UdOverlapMask);
    case 36: return (int)sizeof(UdWarpCamera);       // 35 stays unassigned (-1)
    case 38: return (int)sizeof(UdNormals);          // 37 stays unassigned (-1)
    case 39: return (int)sizeof(UdEvalNormals);
    case 41: return (int)sizeof(UdDepthConsistency); // 40 stays unassigned (-1)
    case 43: return (int)sizeof(UdTsdfIntegrate);    // 42 stays unassigned (-1)
    case 44: return (int)sizeof(UdTsdfPoints);
    case 45: return (int)sizeof(UdTsdfRender);
    case 46: return (int)sizeof(UdTsdfMesh);
    case 48: return (int)sizeof(UdIcp);              // 47 stays unassigned (-1)
    case 49: return (int)sizeof(UdDepthPyramid);
    default: return -1;
  }
}

// numerics bisect / ablation switches: compiled in ONLY for the instrumented tools builds (csrc/build.sh -DUD_TOOLS, used by tools/);
// the product library neither exports ud_set_debug_flags nor reads any switch (ud_debug_flags_host() is a constant 0 there).
#ifdef UD_TOOLS
static int g_debug_flags = 0;
int ud_debug_flags_host() { return g_debug_flags; }
extern "C" void ud_set_debug_flags(int f) { g_debug_flags = f; }
#endif

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is cached per (kernel, device): one process may drive several GPUs.
bool ud_attr_once(bool (&done)[UD_MAX_DEVICES]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= UD_MAX_DEVICES) return false;   // unknown device: set the attribute again
  if (done[dev]) return true;
  done[dev] = true;
  return false;
}
