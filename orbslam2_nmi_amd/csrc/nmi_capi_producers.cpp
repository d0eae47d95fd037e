// nmi_capi_producers.cpp -- C ABI of the stack producers: warp stack, point-cloud and textured-mesh
// render stacks, vertex-coloured-mesh render stacks, the depth renders of clouds and meshes.  Declared in include/nmi_hip.h.
#include "nmi_ctx.h"

using namespace nmi_internal;

namespace nmi_internal {

// Buffers of the mesh renderer (nmi_mesh.hip) for S views: 8 bytes per pixel of visibility keys for the direct path, the
// tile bins (at most 32 MiB) and their state words, the queue of (triangle, view) pairs crossing the near plane.
int mesh_work_alloc(nmi_ctx *ctx, int S, MeshWorkArea *w)
{
    const int width = ctx->params.width, height = ctx->params.height;
    constexpr unsigned long long kClipItems = 1ull << 18;  // beyond it the clip pass rescans the mesh
    *w = MeshWorkArea{};
    NMI_HIP_TRY(ctx, w->zbuf.alloc(nmi::mesh_zbuf_bytes(S, width, height)));
    NMI_HIP_TRY(ctx, w->bins.alloc(nmi::mesh_bins_bytes(S, width, height)));
    NMI_HIP_TRY(ctx, w->state.alloc(nmi::mesh_state_bytes(S, width, height)));
    NMI_HIP_TRY(ctx, w->clip_queue.alloc((size_t)kClipItems * nmi::mesh_clip_item_bytes()));
    NMI_HIP_TRY(ctx, w->clip_state.alloc(2 * sizeof(unsigned long long)));
    NMI_HIP_TRY(ctx, w->pair_state.grow(sizeof(uint32_t), ctx->stream, /*zero=*/true));
    nmi::MeshWork &v = w->view;
    v.zbuf = w->zbuf.as<unsigned long long>();
    v.bins = w->bins.as<uint32_t>();
    v.state = w->state.as<uint32_t>();
    v.clip_queue = w->clip_queue.as<>();
    v.clip_cap = kClipItems;
    v.clip_state = w->clip_state.as<unsigned long long>();
    v.pair_state = w->pair_state.as<uint32_t>();
    v.compute_units = ctx->compute_units;
    NMI_HIP_TRY(ctx, nmi::launch_mesh_clear(v, S, width, height, ctx->stream));
    return NMI_OK;
}

// The pair list of the two-kernel binning pass: 64 entries per block of 256 triangles (grown on demand; a level sizes it once).
int ensure_mesh_pairs(nmi_ctx *ctx, MeshWorkArea *w, long long n_triangles)
{
    const unsigned long long need = nmi::mesh_pairs_entries(n_triangles);
    if (need <= w->view.pairs_cap) return NMI_OK;
    w->view.pairs = nullptr, w->view.pairs_cap = 0;
    if (w->pairs.grow((size_t)need * sizeof(uint32_t), ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return NMI_OK;  // (no list: launch_render_mesh takes the one-kernel form)
    }
    w->view.pairs = w->pairs.as<uint32_t>();
    w->view.pairs_cap = need;
    return NMI_OK;
}

int ensure_mesh_work(nmi_ctx *ctx, int S)
{
    if (S <= ctx->mesh_views) return NMI_OK;
    if (ctx->mesh_views) NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mesh_views = 0;
    const int rc = mesh_work_alloc(ctx, S, &ctx->mesh);
    if (rc != NMI_OK) {
        ctx->mesh = MeshWorkArea{};
        return rc;
    }
    ctx->mesh_views = S;
    return NMI_OK;
}

// warpPerspective inverts the forward matrix on the host in double and hands 9 floats to the device.  A homography is
// defined up to scale, but the floats are not: cast as they come, the inverse of 1e-38 M overflows to inf and that of 1e39 M
// is subnormal, and the determinant of a matrix with entries near 1e-110 underflows to 0.  So M is brought to its largest
// |entry| in [1, 2) before the inversion, and the inverse likewise before the cast.  Both scalings are powers of two: every
// coefficient of a well-scaled matrix keeps its bits up to one common power of two, which the kernels' arithmetic
// (1 / den times a numerator, both linear in the coefficients) cancels exactly -- warps and masks keep their bits.
static void scale_to_unit(double *a)
{
    double mx = 0.0;
    for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(a[i]));
    int e = 0;
    frexp(mx, &e);  // mx = f 2^e, f in [0.5, 1)
    for (int i = 0; i < 9; ++i) a[i] = ldexp(a[i], 1 - e);
}

int warp_inverse_coeffs(const double *forward, float *coeffs)
{
    double m[9];
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(forward[i])) return NMI_ERR_INVALID_ARGUMENT;
        m[i] = forward[i];
    }
    scale_to_unit(m);  // (all zero stays all zero: det == 0 below)
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (det == 0.0) return NMI_ERR_INVALID_ARGUMENT;
    double inv[9] = {(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                     (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                     (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(inv[i])) return NMI_ERR_INVALID_ARGUMENT;  // a subnormal determinant: singular to working precision
    scale_to_unit(inv);
    for (int i = 0; i < 9; ++i) coeffs[i] = (float)inv[i];
    return NMI_OK;
}

// nmi_warp_stack (d_warp_masks null) and nmi_warp_stack_masked: the inverse maps go into a slot of the context's upload ring,
// which is free again after the last kernel that read it.  The masked form's warps are the plain form's, byte for byte.
static int warp_stack_impl(nmi_ctx *ctx, const uint8_t *d_frame, const uint8_t *d_frame_mask, const double *h_forward, int32_t Wn,
                           uint8_t *d_warp_stack, uint8_t *d_warp_masks)
{
    if (!ctx || !d_frame || !h_forward || !d_warp_stack || Wn <= 0) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    nmi_mem::UploadRing::Slot slot;  // (last used four submissions ago; normally long finished)
    NMI_HIP_TRY(ctx, ctx->warp_ring.acquire((size_t)Wn * 9, ctx->stream, &slot));
    for (int w = 0; w < Wn; ++w)
        if (warp_inverse_coeffs(h_forward + (size_t)w * 9, slot.h + (size_t)w * 9) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    NMI_HIP_TRY(ctx, ctx->warp_ring.upload(slot, ctx->stream));
    NMI_HIP_TRY(ctx, nmi::launch_warp(d_frame, slot.d, d_warp_stack, ctx->params.width, ctx->params.height, Wn, ctx->stream));
    if (d_warp_masks)
        NMI_HIP_TRY(ctx, nmi::launch_warp_masks(d_frame_mask, slot.d, d_warp_masks, ctx->params.width, ctx->params.height, Wn, ctx->stream));
    NMI_HIP_TRY(ctx, ctx->warp_ring.release(slot, ctx->stream));
    return NMI_OK;
}

}  // namespace nmi_internal

extern "C" {

// Image::Image warp matrices, image.cpp:76-107: theta_a starts at -(n_a - 1)/2 * step_a with the integer division
// of the reference, advances by step_a; R = Rz*Ry*Rx; M = K * R * K^-1 (doubles).
int nmi_warp_homographies(const double K[9], const int32_t num[3], const float step[3], double *out)
{
    if (!K || !num || !step || !out || num[0] <= 0 || num[1] <= 0 || num[2] <= 0) return NMI_ERR_INVALID_ARGUMENT;
    const double det = K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) + K[2] * (K[3] * K[7] - K[4] * K[6]);
    if (det == 0.0) return NMI_ERR_INVALID_ARGUMENT;
    double Ki[9] = {(K[4] * K[8] - K[5] * K[7]) / det, (K[2] * K[7] - K[1] * K[8]) / det, (K[1] * K[5] - K[2] * K[4]) / det,
                    (K[5] * K[6] - K[3] * K[8]) / det, (K[0] * K[8] - K[2] * K[6]) / det, (K[2] * K[3] - K[0] * K[5]) / det,
                    (K[3] * K[7] - K[4] * K[6]) / det, (K[1] * K[6] - K[0] * K[7]) / det, (K[0] * K[4] - K[1] * K[3]) / det};
    auto mul3 = [](const double *a, const double *b, double *c) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
    };
    const int nx = num[0], ny = num[1], nz = num[2];
    double tz = (double)((float)(-(nz - 1) / 2) * step[2]);
    for (int i = 0; i < nz; ++i, tz += step[2]) {
        const double Rz[9] = {cos(tz), -sin(tz), 0, sin(tz), cos(tz), 0, 0, 0, 1};
        double ty = (double)((float)(-(ny - 1) / 2) * step[1]);
        for (int j = 0; j < ny; ++j, ty += step[1]) {
            const double Ry[9] = {cos(ty), 0, sin(ty), 0, 1, 0, -sin(ty), 0, cos(ty)};
            double tx = (double)((float)(-(nx - 1) / 2) * step[0]);
            for (int k = 0; k < nx; ++k, tx += step[0]) {
                const double Rx[9] = {1, 0, 0, 0, cos(tx), -sin(tx), 0, sin(tx), cos(tx)};
                double t1[9], R[9], t2[9];
                mul3(Rz, Ry, t1);
                mul3(t1, Rx, R);
                mul3(K, R, t2);
                mul3(t2, Ki, out + ((size_t)(i * ny + j) * nx + k) * 9);
            }
        }
    }
    return NMI_OK;
}

int nmi_warp_stack(nmi_ctx *ctx, const uint8_t *d_frame, const double *h_forward, int32_t Wn, uint8_t *d_warp_stack)
{
    return warp_stack_impl(ctx, d_frame, nullptr, h_forward, Wn, d_warp_stack, nullptr);
}

int nmi_warp_stack_masked(nmi_ctx *ctx, const uint8_t *d_frame, const uint8_t *d_frame_mask, const double *h_forward, int32_t Wn,
                          uint8_t *d_warp_stack, uint8_t *d_warp_masks)
{
    if (!d_warp_masks) return NMI_ERR_INVALID_ARGUMENT;
    return warp_stack_impl(ctx, d_frame, d_frame_mask, h_forward, Wn, d_warp_stack, d_warp_masks);
}

// Projection (rendering.hpp:196-202, glm columns) * glm::lookAt(pos + t, look_at + t, up) (rendering.hpp:547-553), fp32.
int nmi_render_mvp(const nmi_render_params *rp, const float cam_pos[3], const float cam_look_at[3], const float cam_up[3],
                   const float translation[3], float out[16])
{
    if (!rp || !cam_pos || !cam_look_at || !cam_up || !translation || !out) return NMI_ERR_INVALID_ARGUMENT;
    const float eye[3] = {cam_pos[0] + translation[0], cam_pos[1] + translation[1], cam_pos[2] + translation[2]};
    const float ctr[3] = {cam_look_at[0] + translation[0], cam_look_at[1] + translation[1], cam_look_at[2] + translation[2]};
    float f[3] = {ctr[0] - eye[0], ctr[1] - eye[1], ctr[2] - eye[2]};
    float len = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(len > 0.0f)) return NMI_ERR_INVALID_ARGUMENT;
    for (float &v : f) v /= len;
    float sv[3] = {f[1] * cam_up[2] - f[2] * cam_up[1], f[2] * cam_up[0] - f[0] * cam_up[2], f[0] * cam_up[1] - f[1] * cam_up[0]};
    len = sqrtf(sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2]);
    if (!(len > 0.0f)) return NMI_ERR_INVALID_ARGUMENT;
    for (float &v : sv) v /= len;
    const float u[3] = {sv[1] * f[2] - sv[2] * f[1], sv[2] * f[0] - sv[0] * f[2], sv[0] * f[1] - sv[1] * f[0]};
    // view matrix, column-major V[c*4 + r]
    float V[16] = {sv[0], u[0], -f[0], 0, sv[1], u[1], -f[1], 0, sv[2], u[2], -f[2], 0, 0, 0, 0, 1};
    V[12] = -(sv[0] * eye[0] + sv[1] * eye[1] + sv[2] * eye[2]);
    V[13] = -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]);
    V[14] = f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2];
    const double zn = rp->near_plane, zf = rp->far_plane;
    float P[16] = {0};
    P[0] = (float)(rp->fx / (-rp->cx));          // Projection[0] = (fx / -cx, 0, 0, 0)
    P[5] = (float)(rp->fy / (-rp->cy));          // Projection[1] = (0, fy / -cy, 0, 0)
    P[10] = (float)((zn + zf) / (zn - zf));      // Projection[2] = (0, 0, (zn+zf)/(zn-zf), -1)
    P[11] = -1.0f;
    P[14] = (float)(2 * zn * zf / (zn - zf));    // Projection[3] = (0, 0, 2 zn zf/(zn-zf), 0)
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            float acc = 0.0f;
            for (int k = 0; k < 4; ++k) acc += P[k * 4 + r] * V[c * 4 + k];
            out[c * 4 + r] = acc;
        }
    return NMI_OK;
}

int nmi_render_points(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                      float point_size, uint8_t *d_render_stack)
{
    return render_points_impl(ctx, d_xyz, d_red, n_points, h_mvps, S, point_size, d_render_stack, nullptr);
}

}  // extern "C"

namespace nmi_internal {

// glPointSize: non-antialiased points use the size rounded to the nearest integer, at least 1 (OpenGL 3.3, 3.4.1), and at most
// the largest supported size (64 here).  The clamp is done in float: converting 1e10, inf or NaN to int is undefined.
int point_sprite_size(float point_size, int *size)
{
    if (std::isnan(point_size)) return NMI_ERR_INVALID_ARGUMENT;
    const float s = floorf(point_size + 0.5f);
    *size = s < 1.0f ? 1 : (s > 64.0f ? 64 : (int)s);
    return NMI_OK;
}

int render_points_impl(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                       float point_size, uint8_t *d_render_stack, uint8_t *cover, const nmi::DepthShade *depth)
{
    if (!ctx || !h_mvps || !d_render_stack || S <= 0 || n_points < 0 || (n_points > 0 && (!d_xyz || (!d_red && !depth))))
        return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    int size = 1;
    if (point_sprite_size(point_size, &size) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && !d_red) {  // a cloud without colours: every point splats colour 0
        NMI_HIP_TRY(ctx, ctx->d_no_red.grow((size_t)n_points * sizeof(float), ctx->stream, /*zero=*/true));
        d_red = ctx->d_no_red.as<float>();
    }
    const int64_t need = (int64_t)nmi::render_zbuf_words(S, ctx->params.width, ctx->params.height, size);
    NMI_HIP_TRY(ctx, ctx->d_zbuf.grow((size_t)need * sizeof(uint32_t), ctx->stream));
    float *d_mvps = nullptr;
    const int src = stage_floats(ctx, ctx->mvp_ring, h_mvps, (size_t)S * 16, &d_mvps);
    if (src != NMI_OK) return src;
    NMI_HIP_TRY(ctx, nmi::launch_render_points(d_xyz, d_red, n_points, nmi::RenderViews{d_mvps, S}, ctx->d_zbuf.as<uint32_t>(), size,
                                               render_target(ctx, d_render_stack, cover, depth), ctx->stream));
    return NMI_OK;
}

int depth_shade_check(const nmi_depth_shade *shade, nmi::DepthShade *out)
{
    if (!shade || !std::isfinite(shade->near_plane) || !std::isfinite(shade->far_plane) || !std::isfinite(shade->scale)) return NMI_ERR_INVALID_ARGUMENT;
    if (!(shade->near_plane > 0.0f) || !(shade->far_plane > shade->near_plane) || !(shade->scale > 0.0f)) return NMI_ERR_INVALID_ARGUMENT;
    if (shade->lo < 0 || shade->lo >= shade->hi || shade->hi > 65535) return NMI_ERR_INVALID_ARGUMENT;
    if (shade->reserved[0] || shade->reserved[1] || shade->reserved[2]) return NMI_ERR_INVALID_ARGUMENT;
    *out = nmi::DepthShade{shade->near_plane, shade->far_plane, shade->scale, (uint32_t)shade->lo, (uint32_t)shade->hi, nullptr};
    return NMI_OK;
}

}  // namespace nmi_internal

// ---------------------------------------------------------------------------------------------------------
// Textured-mesh renderer: texture object (mip chain -> per-level luma on the device) and the draw call.
// ---------------------------------------------------------------------------------------------------------
extern "C" {

int nmi_texture_destroy(nmi_texture *tex)
{
    if (!tex) return NMI_OK;
    DeviceGuard guard(tex->ctx->device);
    (void)hipStreamSynchronize(tex->ctx->stream);
    delete tex;
    return NMI_OK;
}

int nmi_texture_create(nmi_ctx *ctx, const uint8_t *h_rgb, int32_t tw, int32_t th, nmi_texture **out)
{
    if (!ctx || !h_rgb || !out || tw <= 0 || th <= 0 || tw > 32768 || th > 32768) return NMI_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    ctx->detail.clear();
    nmi_texture *tex = new (std::nothrow) nmi_texture;
    if (!tex) return NMI_ERR_INVALID_ARGUMENT;
    tex->ctx = ctx;
    // level sizes: max(1, floor(size / 2)) until 1x1 (OpenGL 3.3, 3.8.14)
    long long total = 0;
    int lw = tw, lh = th;
    for (;;) {
        tex->w[tex->levels] = lw;
        tex->h[tex->levels] = lh;
        tex->off[tex->levels] = total;
        total += (long long)lw * lh;
        ++tex->levels;
        if ((lw == 1 && lh == 1) || tex->levels == 16) break;
        lw = lw > 1 ? lw / 2 : 1;
        lh = lh > 1 ? lh / 2 : 1;
    }
    if (total >= (1ll << 30)) {  // the sampler addresses the pyramid with 32-bit byte offsets (4 bytes per texel)
        delete tex;
        return NMI_ERR_UNSUPPORTED;
    }
    std::vector<uint8_t> cur(h_rgb, h_rgb + (size_t)tw * th * 3), next;
    std::vector<float> luma((size_t)total);
    for (int l = 0; l < tex->levels; ++l) {
        const int w = tex->w[l], h = tex->h[l];
        float *dst = luma.data() + tex->off[l];
        for (size_t i = 0; i < (size_t)w * h; ++i)  // fragment shader :16, on normalised 8-bit channels
            dst[i] = 0.299f * ((float)cur[i * 3] / 255.0f) + 0.587f * ((float)cur[i * 3 + 1] / 255.0f) + 0.114f * ((float)cur[i * 3 + 2] / 255.0f);
        if (l + 1 == tex->levels) break;
        const int nw = tex->w[l + 1], nh = tex->h[l + 1];
        next.assign((size_t)nw * nh * 3, 0);
        for (int y = 0; y < nh; ++y)
            for (int x = 0; x < nw; ++x)
                for (int c = 0; c < 3; ++c) {  // 2x2 box filter, rounded to 8 bits per level
                    const int x0 = 2 * x < w ? 2 * x : w - 1, x1 = 2 * x + 1 < w ? 2 * x + 1 : w - 1;
                    const int y0 = 2 * y < h ? 2 * y : h - 1, y1 = 2 * y + 1 < h ? 2 * y + 1 : h - 1;
                    const int sum = cur[((size_t)y0 * w + x0) * 3 + c] + cur[((size_t)y0 * w + x1) * 3 + c] +
                                    cur[((size_t)y1 * w + x0) * 3 + c] + cur[((size_t)y1 * w + x1) * 3 + c];
                    next[((size_t)y * nw + x) * 3 + c] = (uint8_t)((sum + 2) / 4);
                }
        cur.swap(next);
    }
    DeviceGuard guard(ctx->device);
    hipError_t e = tex->d_luma.alloc((size_t)total * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(tex->d_luma.as<>(), luma.data(), (size_t)total * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const int rc = hip_fail(ctx, e, "nmi_texture_create");
        nmi_texture_destroy(tex);
        return rc;
    }
    *out = tex;
    return NMI_OK;
}

int nmi_render_mesh(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, const nmi_texture *tex,
                    const float *h_mvps, int32_t S, uint8_t *d_render_stack)
{
    return render_mesh_impl(ctx, MapKind::textured_mesh, d_xyz, d_uv, n_triangles, tex, h_mvps, S, d_render_stack, nullptr);
}

int nmi_render_mesh_colored(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const float *h_mvps, int32_t S,
                            uint8_t *d_render_stack)
{
    return render_mesh_impl(ctx, MapKind::colored_mesh, d_xyz, d_red, n_triangles, nullptr, h_mvps, S, d_render_stack, nullptr);
}

int nmi_render_mesh_colored_masked(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, const float *h_mvps,
                                   int32_t S, uint8_t *d_render_stack, uint8_t *d_render_masks)
{
    if (!ctx || !d_render_masks) return NMI_ERR_INVALID_ARGUMENT;
    return render_mesh_impl(ctx, MapKind::colored_mesh, d_xyz, d_red, n_triangles, nullptr, h_mvps, S, d_render_stack, d_render_masks);
}

// The depth renders ("Depth maps", include/nmi_hip.h): the same draws, shaded from the winners' depths.
int nmi_render_points_depth(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, const float *h_mvps, int32_t S,
                            float point_size, const nmi_depth_shade *shade, uint8_t *d_render_stack, uint8_t *d_render_masks, uint16_t *d_depth16)
{
    nmi::DepthShade sh;
    if (depth_shade_check(shade, &sh) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    sh.depth16 = d_depth16;
    return render_points_impl(ctx, d_xyz, d_red, n_points, h_mvps, S, point_size, d_render_stack, d_render_masks, &sh);
}

int nmi_render_mesh_depth(nmi_ctx *ctx, const float *d_xyz, int64_t n_triangles, const float *h_mvps, int32_t S, const nmi_depth_shade *shade,
                          uint8_t *d_render_stack, uint8_t *d_render_masks, uint16_t *d_depth16)
{
    nmi::DepthShade sh;
    if (depth_shade_check(shade, &sh) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    sh.depth16 = d_depth16;
    return render_mesh_impl(ctx, MapKind::colored_mesh, d_xyz, nullptr, n_triangles, nullptr, h_mvps, S, d_render_stack, d_render_masks, &sh);
}

int nmi_depth_shade_apply(nmi_ctx *ctx, const nmi_depth_shade *shade, const uint32_t *d_depth24, int64_t n, uint16_t *d_v, uint8_t *d_grey)
{
    nmi::DepthShade sh;
    if (!ctx || depth_shade_check(shade, &sh) != NMI_OK || n < 0 || (n > 0 && !d_depth24)) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::launch_depth_shade_apply(sh, d_depth24, n, d_v, d_grey, ctx->stream));
    return NMI_OK;
}

}  // extern "C"

namespace nmi_internal {

int render_mesh_impl(nmi_ctx *ctx, MapKind kind, const float *d_xyz, const float *d_attr, int64_t n_triangles, const nmi_texture *tex,
                     const float *h_mvps, int32_t S, uint8_t *d_render_stack, uint8_t *cover, const nmi::DepthShade *depth)
{
    const bool textured = kind == MapKind::textured_mesh;
    if (!ctx || (textured ? (!tex || tex->ctx != ctx) : tex != nullptr) || !h_mvps || !d_render_stack || S <= 0 || n_triangles < 0 ||
        (n_triangles > 0 && (!d_xyz || (!d_attr && !depth))))
        return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    // (the bins' geometry depends on the number of views: a context renders with the work area of its largest stack so far,
    // laid out for that many views; the first S of them are used)
    int rq = ensure_mesh_work(ctx, S);
    if (rq != NMI_OK) return rq;
    if ((rq = ensure_mesh_pairs(ctx, &ctx->mesh, n_triangles)) != NMI_OK) return rq;
    float *d_mvps = nullptr;
    int rc = stage_floats(ctx, ctx->mvp_ring, h_mvps, (size_t)S * 16, &d_mvps);
    if (rc != NMI_OK) return rc;
    const hipError_t e = nmi::launch_render_mesh(d_xyz, mesh_shading(kind, d_attr, tex), n_triangles, nmi::RenderViews{d_mvps, S}, ctx->mesh.view,
                                                 mesh_limits(ctx, ctx->mesh_views), render_target(ctx, d_render_stack, cover, depth), ctx->stream);
    if (e != hipSuccess) {
        ctx->mesh_views = 0;  // whatever state the buffers are in: allocate and clear afresh next time
        return hip_fail(ctx, e, "launch_render_mesh");
    }
    return NMI_OK;
}

nmi::MeshShading mesh_shading(MapKind kind, const float *d_attr, const nmi_texture *tex)
{
    if (kind == MapKind::textured_mesh) return nmi::MeshShading{true, d_attr, tex->d_luma.as<float>(), tex->levels, tex->w, tex->h, tex->off};
    return nmi::MeshShading{false, d_attr};
}

nmi::RenderTarget render_target(const nmi_ctx *ctx, uint8_t *out, uint8_t *cover, const nmi::DepthShade *depth)
{
    nmi::RenderTarget t{};
    t.out = out, t.cover = cover, t.depth = depth;
    t.width = ctx->params.width, t.height = ctx->params.height;
    return t;
}

nmi::MeshLimits mesh_limits(const nmi_ctx *ctx, int layout_views)
{
    nmi::MeshLimits l{};
    l.layout_views = layout_views;
    l.bin_cap = (int)(ctx->tile_queue_limit < 511 ? ctx->tile_queue_limit : 511);
    l.clip_cap = ctx->clip_queue_limit;
    return l;
}

}  // namespace nmi_internal

namespace {

// The argument check of the three nmi_sort_* calls ("Map order", include/nmi_hip.h), before any HIP call: record counts, null
// arrays, and outputs that share a byte with an input or with each other -- at any offset, not only at equal pointers: the gather
// reads whole records of the inputs while other lanes write theirs.  `a` holds na floats per record, `b` nb.
int sort_arguments(const nmi_ctx *ctx, const float *a, int na, const float *b, int nb, int64_t n, const float *a_out, const float *b_out)
{
    if (!ctx || n < 0 || n >= (1ll << 32)) return NMI_ERR_INVALID_ARGUMENT;
    if (n == 0) return NMI_OK;
    if (!a || !b || !a_out || !b_out || a == a_out || b == b_out) return NMI_ERR_INVALID_ARGUMENT;
    const uintptr_t a_bytes = (uintptr_t)n * (uintptr_t)na * sizeof(float), b_bytes = (uintptr_t)n * (uintptr_t)nb * sizeof(float);
    auto meet = [](const float *p, uintptr_t p_bytes, const float *q, uintptr_t q_bytes) {
        const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
        return x < y ? y - x < p_bytes : x - y < q_bytes;
    };
    if (meet(a_out, a_bytes, a, a_bytes) || meet(a_out, a_bytes, b, b_bytes) || meet(b_out, b_bytes, a, a_bytes) ||
        meet(b_out, b_bytes, b, b_bytes) || meet(a_out, a_bytes, b_out, b_bytes))
        return NMI_ERR_INVALID_ARGUMENT;
    return NMI_OK;
}

int sort_map(nmi_ctx *ctx, const float *a, int na, int verts, const float *b, int nb, int64_t n, float *a_out, float *b_out)
{
    const int rc = sort_arguments(ctx, a, na, b, nb, n, a_out, b_out);
    if (rc != NMI_OK) return rc;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::sort_records_morton(a, na, verts, b, nb, n, a_out, b_out, ctx->stream));
    return NMI_OK;
}

}  // namespace

extern "C" {

int nmi_sort_points(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_points, float *d_xyz_out, float *d_red_out)
{
    return sort_map(ctx, d_xyz, 3, 1, d_red, 1, n_points, d_xyz_out, d_red_out);
}

int nmi_sort_triangles(nmi_ctx *ctx, const float *d_xyz, const float *d_uv, int64_t n_triangles, float *d_xyz_out, float *d_uv_out)
{
    return sort_map(ctx, d_xyz, 9, 3, d_uv, 6, n_triangles, d_xyz_out, d_uv_out);
}

int nmi_sort_triangles_colored(nmi_ctx *ctx, const float *d_xyz, const float *d_red, int64_t n_triangles, float *d_xyz_out, float *d_red_out)
{
    return sort_map(ctx, d_xyz, 9, 3, d_red, 3, n_triangles, d_xyz_out, d_red_out);
}

}  // extern "C"
