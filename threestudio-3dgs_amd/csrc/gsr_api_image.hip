// gsr_api_image.hip — the image-space entry points of include/gsr.h: composite, normal map and the shading epilogue
// (kernels: gsr_epilogue.hip, gsr_shading.hip).
#include <vector>

#include "gsr_api.h"

using namespace gsr;

extern "C" {

int gsr_composite_forward(int V, int height, int width, const float* color, const float* alpha, const float* bg,
                          int bg_layout, float* out, void* stream) {
  if (V < 0 || height < 0 || width < 0 || bg_layout < 0 || bg_layout > 2) return invalid("bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (color == nullptr || alpha == nullptr || bg == nullptr || out == nullptr) return null_argument();
  launch_composite_fwd(V, (size_t)height * width, color, alpha, bg, bg_layout, out, (hipStream_t)stream);
  return last_launch();
}

int gsr_composite_backward(int V, int height, int width, const float* dL_dout, const float* color,
                           const float* alpha, const float* bg, int bg_layout, float* dL_dcolor, float* dL_dalpha,
                           float* dL_dbg, void* stream) {
  if (V < 0 || height < 0 || width < 0 || bg_layout < 0 || bg_layout > 2) return invalid("bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (dL_dout == nullptr || color == nullptr || alpha == nullptr || bg == nullptr || dL_dcolor == nullptr ||
      dL_dalpha == nullptr)
    return null_argument();
  if (dL_dbg != nullptr && bg_layout == GSR_BG_CONSTANT)
    return invalid("dL_dbg is computed for image backgrounds only");
  launch_composite_bwd(V, (size_t)height * width, dL_dout, color, alpha, bg, bg_layout, dL_dcolor, dL_dalpha,
                       dL_dbg, (hipStream_t)stream);
  return last_launch();
}

int gsr_normal_map_forward(int V, int height, int width, const float* normal, const float* alpha, float* out,
                           void* stream) {
  if (V < 0 || height < 0 || width < 0) return invalid("bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (normal == nullptr || alpha == nullptr || out == nullptr) return null_argument();
  launch_normal_map_fwd(V, (size_t)height * width, normal, alpha, out, (hipStream_t)stream);
  return last_launch();
}

int gsr_normal_map_backward(int V, int height, int width, const float* dL_dout, const float* normal,
                            const float* alpha, float* dL_dnormal, float* dL_dalpha, void* stream) {
  if (V < 0 || height < 0 || width < 0) return invalid("bad sizes");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  if (dL_dout == nullptr || normal == nullptr || alpha == nullptr || dL_dnormal == nullptr || dL_dalpha == nullptr)
    return null_argument();
  launch_normal_map_bwd(V, (size_t)height * width, dL_dout, normal, alpha, dL_dnormal, dL_dalpha, (hipStream_t)stream);
  return last_launch();
}

static int shade_args(int V, int H, int W, int flags, const int* modes, const float* color, const float* depth,
                      const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                      const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                      ShadeArgs& A) {
  if (V < 0 || H < 0 || W < 0 || (flags & ~GSR_SHADE_MATERIAL) != 0) return invalid("bad sizes / flags");
  if (depth == nullptr || alpha == nullptr || rays_o == nullptr || rays_d == nullptr)
    return invalid("null pointer argument (depth / alpha / rays)");
  A = ShadeArgs{};
  A.V = V, A.H = H, A.W = W, A.flags = flags, A.bg_layout = bg_layout;
  A.color = color, A.depth = depth, A.alpha = alpha, A.rays_o = rays_o, A.rays_d = rays_d;
  A.bg = bg, A.light = light, A.pred_normal = pred_normal;
  if (flags & GSR_SHADE_MATERIAL) {
    if (color == nullptr || bg == nullptr || light == nullptr || ambient == nullptr || diffuse == nullptr ||
        modes == nullptr)
      return invalid("material: color, bg, light, ambient, diffuse and modes are required");
    if (bg_layout != GSR_BG_CONSTANT && bg_layout != GSR_BG_HWC)
      return invalid("material: bg_layout must be GSR_BG_CONSTANT or GSR_BG_HWC");
    for (int v = 0; v < V; ++v)
      if (modes[v] < GSR_SHADING_DIFFUSE || modes[v] > GSR_SHADING_TEXTURELESS) return invalid("bad shading mode");
  }
  return GSR_OK;
}

// Launches in chunks of GSR_SET_MAX views, each with its views' light colours and modes in the arguments.
static void shade_launch(ShadeArgs A, const ShadeGrads* G, const int* modes, const float* ambient,
                         const float* diffuse, hipStream_t s) {
  const int V = A.V;
  for (int v0 = 0; v0 < V; v0 += GSR_SET_MAX) {
    const int n = V - v0 < GSR_SET_MAX ? V - v0 : GSR_SET_MAX;
    A.v0 = v0, A.V = n;
    for (int i = 0; i < n; ++i) {
      A.mode[i] = (A.flags & GSR_SHADE_MATERIAL) ? modes[v0 + i] : 0;
      for (int k = 0; k < 3; ++k) {
        A.ka[i][k] = (A.flags & GSR_SHADE_MATERIAL) ? ambient[3 * (v0 + i) + k] : 0.0f;
        A.kd[i][k] = (A.flags & GSR_SHADE_MATERIAL) ? diffuse[3 * (v0 + i) + k] : 0.0f;
      }
    }
    if (G == nullptr)
      launch_shade_fwd(A, s);
    else
      launch_shade_bwd(A, *G, s);
  }
}

int gsr_shade_views_forward(int V, int height, int width, int flags, const int* modes, const float* color,
                            const float* depth, const float* alpha, const float* rays_o, const float* rays_d,
                            const float* bg, int bg_layout, const float* light, const float* pred_normal,
                            const float* ambient, const float* diffuse, float* render, float* normal_map,
                            float* unit_normal, float* depth_out, void* stream) {
  ShadeArgs A;
  if (shade_args(V, height, width, flags, modes, color, depth, alpha, rays_o, rays_d, bg, bg_layout, light,
                 pred_normal, ambient, diffuse, A) != GSR_OK)
    return GSR_EINVAL;
  if ((flags & GSR_SHADE_MATERIAL) && render == nullptr) return invalid("material: render output is required");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  A.render = render, A.nmap = normal_map, A.unit = unit_normal, A.depth_out = depth_out;
  shade_launch(A, nullptr, modes, ambient, diffuse, (hipStream_t)stream);
  return last_launch();
}

int gsr_shade_views_backward(int V, int height, int width, int flags, const int* modes, const float* color,
                             const float* depth, const float* alpha, const float* rays_o, const float* rays_d,
                             const float* bg, int bg_layout, const float* light, const float* pred_normal,
                             const float* ambient, const float* diffuse, const float* dL_drender,
                             const float* dL_dnormal_map, const float* dL_dunit_normal, const float* dL_ddepth_out,
                             float* dL_dcolor, float* dL_ddepth, float* dL_dalpha, float* dL_dbg, void* stream) {
  ShadeArgs A;
  if (shade_args(V, height, width, flags, modes, color, depth, alpha, rays_o, rays_d, bg, bg_layout, light,
                 pred_normal, ambient, diffuse, A) != GSR_OK)
    return GSR_EINVAL;
  if (dL_ddepth == nullptr || dL_dalpha == nullptr) return invalid("dL_ddepth / dL_dalpha required");
  if ((flags & GSR_SHADE_MATERIAL) && dL_dcolor == nullptr) return invalid("material: dL_dcolor is required");
  if (dL_dbg != nullptr && !((flags & GSR_SHADE_MATERIAL) && bg_layout == GSR_BG_HWC))
    return invalid("dL_dbg is formed for GSR_BG_HWC material shading only");
  if (V == 0 || height == 0 || width == 0) return last_launch();
  ShadeGrads G{dL_drender, dL_dnormal_map, dL_dunit_normal, dL_ddepth_out, dL_dcolor, dL_ddepth, dL_dalpha, dL_dbg};
  shade_launch(A, &G, modes, ambient, diffuse, (hipStream_t)stream);
  return last_launch();
}

// one (ambient, diffuse, mode) for every view: the per-view tables filled with copies
struct SharedLight {
  std::vector<int> modes;
  std::vector<float> ka, kd;
  SharedLight(int V, int mode, const float* ambient, const float* diffuse)
      : modes(V > 0 ? V : 0, mode), ka(3 * (size_t)(V > 0 ? V : 0)), kd(3 * (size_t)(V > 0 ? V : 0)) {
    for (int v = 0; v < V; ++v)
      for (int k = 0; k < 3; ++k) {
        ka[3 * v + k] = ambient ? ambient[k] : 0.0f;
        kd[3 * v + k] = diffuse ? diffuse[k] : 0.0f;
      }
  }
  // what gsr_shade_forward and gsr_shade_backward check before they build one (it reads ambient and diffuse)
  static int check(int V, int flags, int mode, const float* ambient, const float* diffuse) {
    if (V < 0 || V > 65535 || mode < 0 || mode > 2) return invalid("bad sizes / mode / flags");
    if ((flags & GSR_SHADE_MATERIAL) && (ambient == nullptr || diffuse == nullptr))
      return invalid("material: color, bg, light, ambient, diffuse and modes are required");
    return GSR_OK;
  }
};

int gsr_shade_forward(int V, int height, int width, int flags, int mode, const float* color, const float* depth,
                      const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                      const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                      float* render, float* normal_map, float* unit_normal, float* depth_out, void* stream) {
  if (SharedLight::check(V, flags, mode, ambient, diffuse) != GSR_OK) return GSR_EINVAL;
  SharedLight L(V, mode, ambient, diffuse);
  return gsr_shade_views_forward(V, height, width, flags, L.modes.data(), color, depth, alpha, rays_o, rays_d, bg,
                                 bg_layout, light, pred_normal, L.ka.data(), L.kd.data(), render, normal_map,
                                 unit_normal, depth_out, stream);
}

int gsr_shade_backward(int V, int height, int width, int flags, int mode, const float* color, const float* depth,
                       const float* alpha, const float* rays_o, const float* rays_d, const float* bg, int bg_layout,
                       const float* light, const float* pred_normal, const float* ambient, const float* diffuse,
                       const float* dL_drender, const float* dL_dnormal_map, const float* dL_dunit_normal,
                       const float* dL_ddepth_out, float* dL_dcolor, float* dL_ddepth, float* dL_dalpha,
                       float* dL_dbg, void* stream) {
  if (SharedLight::check(V, flags, mode, ambient, diffuse) != GSR_OK) return GSR_EINVAL;
  SharedLight L(V, mode, ambient, diffuse);
  return gsr_shade_views_backward(V, height, width, flags, L.modes.data(), color, depth, alpha, rays_o, rays_d, bg,
                                  bg_layout, light, pred_normal, L.ka.data(), L.kd.data(), dL_drender,
                                  dL_dnormal_map, dL_dunit_normal, dL_ddepth_out, dL_dcolor, dL_ddepth, dL_dalpha,
                                  dL_dbg, stream);
}

}  // extern "C"
