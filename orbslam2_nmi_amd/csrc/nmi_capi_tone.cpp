// nmi_capi_tone.cpp -- the tone map of the deep grey frames (NMI_FRAME_GRAY16, include/nmi_hip.h): nmi_tone_map_default,
// nmi_set_tone_map, nmi_set_valid_range, nmi_tone_lut, nmi_tone_tile_luts, nmi_deep_frame, nmi_unpack_frame (the container of a
// packed, big-endian or mosaic deep source: nmi_unpack.h) with nmi_frame_row_bytes, and the host side every GRAY16
// conversion shares (nmi_tone.h): the check of a setting, the buffers that go with it and the nodes in front of the conversion.  nmi_level_set_tone_map and
// nmi_stream_set_tone_map are with the other setters in nmi_capi_pipeline.cpp.  Kernels: nmi_tone.hip, and nmi_clahe.hip for the
// tiled mode.
#include "nmi_tone.h"

#include "nmi_color.h"
#include "nmi_ctx.h"
#include "nmi_unpack.h"

using namespace nmi_internal;

int nmi_internal::tone_check(const nmi_tone_map *tm, int width, int height, nmi::ToneSetting *out)
{
    nmi::ToneSetting t;  // (the default: SHIFT, 16 bits)
    if (tm) {
        if (tm->bits < 8 || tm->bits > 16) return NMI_ERR_INVALID_ARGUMENT;
        // the tile counts were reserved words: 0 under every mode but CLAHE
        if (tm->mode != NMI_TONE_CLAHE && (tm->tiles_x != 0 || tm->tiles_y != 0)) return NMI_ERR_INVALID_ARGUMENT;
        for (int32_t r : tm->reserved)
            if (r != 0) return NMI_ERR_INVALID_ARGUMENT;
        const int32_t M = (1 << tm->bits) - 1;
        t.mode = tm->mode;
        t.bits = tm->bits;
        t.hi = M;
        switch (tm->mode) {
        case NMI_TONE_SHIFT: break;
        case NMI_TONE_WINDOW:
            if (tm->lo < 0 || tm->lo >= tm->hi || tm->hi > M) return NMI_ERR_INVALID_ARGUMENT;
            t.lo = tm->lo, t.hi = tm->hi;
            break;
        case NMI_TONE_PERCENTILE:
            if (tm->p_lo < 0 || tm->p_hi < 0 || (int64_t)tm->p_lo + tm->p_hi >= 10000) return NMI_ERR_INVALID_ARGUMENT;
            t.p_lo = tm->p_lo, t.p_hi = tm->p_hi;
            break;
        case NMI_TONE_EQUALIZE:
            if (tm->plateau < 0) return NMI_ERR_INVALID_ARGUMENT;
            t.plateau = tm->plateau;
            break;
        case NMI_TONE_TABLE:
            if (!tm->d_lut) return NMI_ERR_INVALID_ARGUMENT;
            t.d_lut = tm->d_lut;
            break;
        case NMI_TONE_CLAHE:
            if (tm->plateau < 0 || tm->tiles_x < 1 || tm->tiles_x > nmi::kClaheMaxTiles || tm->tiles_y < 1 || tm->tiles_y > nmi::kClaheMaxTiles ||
                tm->tiles_x > width || tm->tiles_y > height)
                return NMI_ERR_INVALID_ARGUMENT;
            t.plateau = tm->plateau;
            t.tiles_x = tm->tiles_x, t.tiles_y = tm->tiles_y;
            break;
        default: return NMI_ERR_INVALID_ARGUMENT;
        }
    }
    *out = t;
    return NMI_OK;
}

size_t nmi_internal::container_bytes(int32_t format, int factor, int width, int height)
{
    return nmi::frame_needs_unpack(format) ? 2 * ((size_t)factor * width) * ((size_t)factor * height) : 0;
}

hipError_t nmi_internal::tone_prepare(ToneWork *w, const nmi::ToneSetting &t, hipStream_t stream, size_t container)
{
    const size_t lut_bytes = (size_t)nmi::kToneLevels + 2 * sizeof(int32_t);
    if (w->lut.size() < lut_bytes) w->built = false;
    hipError_t e = container ? w->container.grow(container, stream) : hipSuccess;
    if (e != hipSuccess) return e;
    e = w->lut.grow(lut_bytes, stream);
    if (e != hipSuccess || t.mode == NMI_TONE_TABLE) return e;
    if (t.tiled()) {  // the tiles' histograms start clean and the table kernel leaves them so; a setting of fewer bits or tiles fits
        w->built = false;
        e = w->tile_luts.grow(nmi::clahe_luts_bytes(t) + nmi::kClaheMaxTileCount * sizeof(uint32_t), stream);
        return e != hipSuccess ? e : w->tile_hist.grow(nmi::clahe_hist_bytes(t), stream, /*zero=*/true);
    }
    if (t.from_frame()) {  // the table is each frame's own; the histogram starts clean and every table kernel leaves it so
        w->built = false;
        return w->hist.grow(nmi::kToneHistWords * sizeof(uint32_t), stream, /*zero=*/true);
    }
    if (w->built && w->fixed == t) return hipSuccess;
    e = nmi::launch_tone_table(t, nullptr, w->table(), w->window(), stream);
    w->built = e == hipSuccess;
    w->fixed = t;
    return e;
}

int nmi_internal::valid_range_check(int32_t lo, int32_t hi, nmi::ValidRange *out)
{
    if (lo < 0 || lo > hi || hi > 65535) return NMI_ERR_INVALID_ARGUMENT;
    out->lo = lo, out->hi = hi;
    return NMI_OK;
}

hipError_t nmi_internal::launch_tone(const ToneWork &w, const nmi::ToneSetting &t, const nmi::ValidRange &range, const uint8_t *src,
                                     int64_t pitch, int width, int height, const uint8_t **lut, hipStream_t stream)
{
    *lut = t.mode == NMI_TONE_TABLE ? t.d_lut : w.table();
    if (!t.from_frame()) return hipSuccess;
    const hipError_t e = nmi::launch_tone_hist(src, pitch, width, height, t.bits, range, w.hist.as<uint32_t>(), stream);
    return e != hipSuccess ? e : nmi::launch_tone_table(t, w.hist.as<uint32_t>(), w.table(), w.window(), stream);
}

hipError_t nmi_internal::launch_clahe_tone(const ToneWork &w, const nmi::ToneSetting &t, const nmi::ValidRange &range, const uint8_t *src,
                                           int64_t pitch, int width, int height, hipStream_t stream)
{
    const hipError_t e = nmi::launch_clahe_hist(t, src, pitch, width, height, range, w.tile_hist.as<uint32_t>(), stream);
    return e != hipSuccess ? e : nmi::launch_clahe_tables(t, w.tile_hist.as<uint32_t>(), w.tile_tables(), w.tile_counts(t), stream);
}

hipError_t nmi_internal::deep_gray(const ToneWork &w, const nmi::ToneSetting &t, const nmi::ValidRange &range, const uint8_t *src, int format,
                                   int64_t pitch, int factor, const uint8_t *frame_mask, uint8_t *gray, uint8_t *mask_out, int width,
                                   int height, hipStream_t stream)
{
    if (format != NMI_FRAME_GRAY16) {  // the container first; from here on the source is dense GRAY16
        if (w.container.size() < container_bytes(format, factor, width, height) || !w.container) return hipErrorInvalidValue;
        const hipError_t e = nmi::launch_unpack(src, format, pitch, w.container.as<uint16_t>(), factor * width, factor * height, stream);
        if (e != hipSuccess) return e;
        src = w.container.as<uint8_t>();
        pitch = 2 * (int64_t)factor * width;
    }
    if (t.tiled()) {
        const hipError_t e = launch_clahe_tone(w, t, range, src, pitch, factor * width, factor * height, stream);
        if (e != hipSuccess) return e;
        return nmi::launch_clahe_gray16(t, src, pitch, factor, w.tile_tables(), range, frame_mask, gray, mask_out, width, height, stream);
    }
    const uint8_t *lut = nullptr;
    const hipError_t e = launch_tone(w, t, range, src, pitch, factor * width, factor * height, &lut, stream);
    if (e != hipSuccess) return e;
    return nmi::launch_gray16(src, pitch, factor, lut, t.bits, range, frame_mask, gray, mask_out, width, height, stream);
}

namespace {

// nmi_tone_lut's and nmi_tone_tile_luts' arguments: the f W x f H GRAY16 source, and `bytes` of table at d_out that may not
// meet the source's bytes.  NMI_OK: *src.
int tone_source_check(const nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch, int32_t factor, const uint8_t *d_out, size_t bytes, FrameSource *src)
{
    if (!ctx || !d_src || !d_out) return NMI_ERR_INVALID_ARGUMENT;
    if (frame_source_check(NMI_FRAME_GRAY16, pitch, factor, ctx->params.width, ctx->params.height, d_src, src) != NMI_OK)
        return NMI_ERR_INVALID_ARGUMENT;
    return meet(span_of(d_out, bytes), src->bytes) ? NMI_ERR_INVALID_ARGUMENT : NMI_OK;
}

}  // namespace

extern "C" {

int nmi_tone_map_default(nmi_tone_map *tm)
{
    if (!tm) return NMI_ERR_INVALID_ARGUMENT;
    *tm = nmi_tone_map{};
    tm->mode = NMI_TONE_SHIFT;
    tm->bits = 16;
    tm->hi = 65535;
    return NMI_OK;
}

int nmi_set_tone_map(nmi_ctx *ctx, const nmi_tone_map *tm)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    return tone_check(tm, ctx->params.width, ctx->params.height, &ctx->tone);
}

int nmi_set_valid_range(nmi_ctx *ctx, int32_t lo, int32_t hi)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    return valid_range_check(lo, hi, &ctx->valid);
}

int nmi_tone_lut(nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch, int32_t factor, uint8_t *d_lut, int32_t h_window[2])
{
    FrameSource src;
    if (tone_source_check(ctx, d_src, pitch, factor, d_lut, nmi::kToneLevels, &src) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    const nmi::ToneSetting t = ctx->tone;
    if (t.tiled()) return NMI_ERR_UNSUPPORTED;  // no single table: nmi_tone_tile_luts
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    ToneWork &w = ctx->tone_work;
    NMI_HIP_TRY(ctx, tone_prepare(&w, t, ctx->stream));
    if (t.from_frame()) NMI_HIP_TRY(ctx, nmi::launch_tone_hist(d_src, src.row_bytes, src.width, src.height, t.bits, ctx->valid, w.hist.as<uint32_t>(), ctx->stream));
    NMI_HIP_TRY(ctx, nmi::launch_tone_table(t, w.hist.as<uint32_t>(), d_lut, w.window(), ctx->stream));
    if (h_window) {
        NMI_HIP_TRY(ctx, hipMemcpyAsync(h_window, w.window(), 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return NMI_OK;
}

int nmi_tone_tile_luts(nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch, int32_t factor, uint8_t *d_luts, int32_t *h_counts)
{
    if (!ctx) return NMI_ERR_INVALID_ARGUMENT;
    const nmi::ToneSetting t = ctx->tone;
    const size_t bytes = t.tiled() ? nmi::clahe_luts_bytes(t) : (size_t)nmi::kToneLevels;
    FrameSource src;
    if (tone_source_check(ctx, d_src, pitch, factor, d_luts, bytes, &src) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    if (!t.tiled()) return NMI_ERR_UNSUPPORTED;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    ToneWork &w = ctx->tone_work;
    NMI_HIP_TRY(ctx, tone_prepare(&w, t, ctx->stream));
    NMI_HIP_TRY(ctx, nmi::launch_clahe_hist(t, d_src, src.row_bytes, src.width, src.height, ctx->valid, w.tile_hist.as<uint32_t>(), ctx->stream));
    NMI_HIP_TRY(ctx, nmi::launch_clahe_tables(t, w.tile_hist.as<uint32_t>(), d_luts, w.tile_counts(t), ctx->stream));
    if (h_counts) {
        NMI_HIP_TRY(ctx, hipMemcpyAsync(h_counts, w.tile_counts(t), (size_t)t.tiles_x * t.tiles_y * sizeof(int32_t), hipMemcpyDeviceToHost,
                                        ctx->stream));
        NMI_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return NMI_OK;
}

int nmi_deep_frame(nmi_ctx *ctx, const uint8_t *d_src, int64_t pitch, int32_t factor, const uint8_t *d_frame_mask, uint8_t *d_gray,
                   uint8_t *d_mask)
{
    if (!ctx || !d_src || !d_gray || !d_mask) return NMI_ERR_INVALID_ARGUMENT;
    const int W = ctx->params.width, H = ctx->params.height;
    FrameSource src;
    if (frame_source_check(NMI_FRAME_GRAY16, pitch, factor, W, H, d_src, &src) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    // the frame mask and the two outputs are dense [H][W]; no two of the four may meet (a NULL frame mask meets nothing)
    const Span spans[4] = {src.bytes, span_of(d_frame_mask, ctx->npix), span_of(d_gray, ctx->npix), span_of(d_mask, ctx->npix)};
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (meet(spans[a], spans[b])) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    const nmi::ToneSetting t = ctx->tone;
    const nmi::ValidRange range = ctx->valid;
    NMI_HIP_TRY(ctx, tone_prepare(&ctx->tone_work, t, ctx->stream));
    // (range off: every pixel is valid, and the masked conversion writes the frame mask as 0 / 1, all 1 without one)
    NMI_HIP_TRY(ctx, deep_gray(ctx->tone_work, t, range, d_src, NMI_FRAME_GRAY16, src.row_bytes, factor, d_frame_mask, d_gray, d_mask, W, H, ctx->stream));
    return NMI_OK;
}

int64_t nmi_frame_row_bytes(int32_t format, int32_t width) { return frame_row_bytes(format, width); }

int nmi_unpack_frame(nmi_ctx *ctx, const uint8_t *d_src, int32_t format, int64_t pitch, int32_t factor, uint16_t *d_gray16)
{
    if (!ctx || !d_src || !d_gray16 || !nmi::frame_needs_unpack(format) || ((uintptr_t)d_gray16 % 2) != 0) return NMI_ERR_INVALID_ARGUMENT;
    FrameSource src;
    if (frame_source_check(format, pitch, factor, ctx->params.width, ctx->params.height, d_src, &src) != NMI_OK) return NMI_ERR_INVALID_ARGUMENT;
    // the container's 2 f W f H bytes may not meet the source's
    if (meet(span_of(d_gray16, 2 * (size_t)src.width * src.height), src.bytes)) return NMI_ERR_INVALID_ARGUMENT;
    ctx->detail.clear();
    DeviceGuard guard(ctx->device);
    NMI_HIP_TRY(ctx, nmi::launch_unpack(d_src, format, src.row_bytes, d_gray16, src.width, src.height, ctx->stream));
    return NMI_OK;
}

}  // extern "C"
