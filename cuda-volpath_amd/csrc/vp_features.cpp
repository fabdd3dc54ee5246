// vp_features.cpp -- the feature pass (include/volpath.h vp_render_features): the argument checks, the per-view tables and pixel lists
// as vp_prepare builds them, then the class fills and the march (vp_kernels.hip features_fill_k, features_k).  A pass of its own beside
// the render path: it reads the context's scene, tables and lists and writes the caller's two buffers, nothing else.
#include "vp_state.h"

static_assert(sizeof(vp_feature_params) == 8, "vp_feature_params layout (include/volpath.h)");

using namespace vph;

int vp_render_features(vp_float4* d_alpha, vp_float4* d_depth, const Param* p, const vp_feature_params* fp)
{
    // ---- what can be refused from the arguments and the host's state: before the device is touched
    if (!d_alpha || !d_depth || !p || !fp) return fail(VP_E_ARG, "vp_render_features: null argument");
    if (d_alpha == d_depth) return fail(VP_E_ARG, "vp_render_features: alpha and depth are one buffer");
    if (!std::isfinite(fp->step) || !(fp->step > 0.0f)) return fail(VP_E_ARG, "vp_render_features: step %g is not a finite number > 0", (double)fp->step);
    if (!std::isfinite(fp->tau_z) || !(fp->tau_z > 0.0f)) return fail(VP_E_ARG, "vp_render_features: tau_z %g is not a finite number > 0", (double)fp->tau_z);
    if (p->width < 1 || p->height < 1 || p->width > 65535 || p->height > 65535) return fail(VP_E_ARG, "image %ux%u out of range", p->width, p->height);
    if (!G.have_volume || !G.have_cam) return fail(VP_E_STATE, "vp_render_features needs a volume and a camera");
    if (G.sub_shift) return fail(VP_E_STATE, "vp_render_features is not built for a sub-pixel factor above 1 (the mean of depths that may be infinite is another definition)");
    {
        // no chord is longer than the box diagonal: in binary64, from the box
        double d2 = 0.0;
        for (int a = 0; a < 3; a++) { const double e = (double)G.S.bmax[a] - (double)G.S.bmin[a]; d2 += e * e; }
        const double steps = std::sqrt(d2) / (double)fp->step;
        if (!(steps <= (double)VP_FEATURE_MAX_STEPS))
            return fail(VP_E_ARG, "vp_render_features: step %g takes %.0f steps across the box diagonal (at most %u)", (double)fp->step, steps, VP_FEATURE_MAX_STEPS);
    }
    int rc = ensure_device();
    if (rc) return rc;
    const Shard sh = shard_of(p);
    if (sh.per_frame == 0) return VP_OK;   // a shard without a tile
    // ---- the per-view table and the lists of this context, found cached where a render or vp_prepare of this view built them
    const float4* table = nullptr;
    if ((rc = ensure_crawl_table(p, &table))) return rc;
    if ((rc = ensure_pixel_lists(p, table, sh))) return rc;
    FeatureDev F;
    F.width = p->width; F.height = p->height;
    F.step = fp->step; F.tau_z = fp->tau_z; F.density = p->density;
    F.sigma_t[0] = p->sigma_t.x; F.sigma_t[1] = p->sigma_t.y; F.sigma_t[2] = p->sigma_t.z;
    F.alpha = (float4*)d_alpha; F.depth = (float4*)d_depth;
    SceneDev S = G.S;
    S.linear   = G.linear ? 1 : 0;
    if (!G.use_feature_skip)
    {
        // every owned pixel marches its whole chord (a ray that misses the box has none)
        F.pixels = G.d_tiles; F.n = G.n_general + G.n_light + G.n_miss; F.table = nullptr;
        launch_features(S, G.quant, G.vol_format == VP_VOL_F16, F, G.stream);
        HIPCHK(hipGetLastError());
        return VP_OK;
    }
    if (G.n_light + G.n_miss)
    {
        F.pixels = G.d_tiles + G.n_general; F.n = G.n_light + G.n_miss; F.table = nullptr;
        launch_features_fill(F, G.n_light, G.stream);
        HIPCHK(hipGetLastError());
    }
    if (G.n_general)
    {
        F.pixels = G.d_tiles; F.n = G.n_general; F.table = table;
        launch_features(S, G.quant, G.vol_format == VP_VOL_F16, F, G.stream);
        HIPCHK(hipGetLastError());
    }
    return VP_OK;
}
