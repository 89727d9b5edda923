// stream_abi.cpp -- mvhp_stream_* entry points of include/minivideo_hotpath.h:
// Annex-B buffer -> sample table -> parameter sets -> packed pictures (host only).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../hip/resample_taps.h"
#include "bars_policy.h"
#include "h264_frontend.h"
#include "mp4_demux.h"
#include "stream_internal.h"
#include "tensor_policy.h"

using namespace h264;

// A slice cannot be smaller than its picture allows: a CAVLC macroblock takes at least one bit, a CABAC one rarely
// less than a quarter of a bit -- eight macroblocks per payload bit is far outside anything an encoder emits.  Checked
// before any picture-sized buffer is reserved, so a 100-byte file announcing 1024 x 1024 macroblocks costs nothing.
static bool slice_can_hold_picture(const Sps &sps, size_t nal_size)
{
    return (uint64_t)nal_size * 64u >= (uint64_t)sps.width_mbs * (uint64_t)sps.height_map_units;
}

int mvhp_stream::build(std::string &err)
{
    if ((spec ? index_annexb_spec(data, size, samples) : index_annexb(data, size, samples)) != RC_SUCCESS) { err = "no NAL unit found in the bitstream"; return RC_FAILURE; }
    Sps sps_tab[32];
    Pps pps_tab[256];
    std::vector<uint8_t> rbsp;
    for (size_t i = 0; i < samples.size(); i++) {
        const EsSample &s = samples[i];
        if (s.nal_size < 2) continue;
        // (of a slice only first_mb_in_slice, slice_type and pic_parameter_set_id are read here: three ue(v) of at most 65
        // bits each -- the picture's 200 KB are unescaped by the thread that decodes it, not by this loop)
        unescape_rbsp(data + s.offset + 1, s.nal_unit_type == 5 ? std::min<size_t>(s.nal_size - 1, 64) : s.nal_size - 1, rbsp);
        BitReader br(rbsp.data(), rbsp.size());
        std::string e;
        if (s.nal_unit_type == 7) {
            Sps sps;
            if (parse_sps(br, sps, e, spec) == RC_SUCCESS) sps_tab[sps.sps_id] = sps;
            else param_errors++;
        } else if (s.nal_unit_type == 8) {
            Pps pps;
            if (parse_pps(br, sps_tab, pps, e, spec) == RC_SUCCESS) pps_tab[pps.pps_id] = pps;
            else param_errors++;
        } else if (s.nal_unit_type == 5) {
            Idr idr;
            idr.sample = i;
            const unsigned first_mb = br.ue(); // first_mb_in_slice (the reference ignores it, h264_slice.c:1019)
            br.ue(); // slice_type
            const unsigned pid = br.ue();
            if (pid < 256 && pps_tab[pid].valid && sps_tab[pps_tab[pid].sps_id].valid) {
                idr.pps = pps_tab[pid];
                idr.sps = sps_tab[idr.pps.sps_id];
                // reference mode: one slice NAL = one picture, and it must be able to hold it.  MVHP_STREAM_SPEC: a picture may
                // come in many small slices (one per macroblock row of flat content: ten bytes each) -- the guard goes by the
                // bytes of ALL its slices, once the last one is known (below)
                idr.nal_bytes = s.nal_size;
                idr.ok = spec || slice_can_hold_picture(idr.sps, s.nal_size);
                if (!idr.ok) idr.why = "slice NAL too small for the picture size of its SPS";
                if (spec && first_mb != 0) {   // a further slice of the previous picture: not a picture of its own
                    if (idrs.empty()) continue;                       // (a stream that starts in the middle of a picture)
                    Idr &pic = idrs.back();
                    if (pic.ok && pic.pps.pps_id != (int)pid) { pic.ok = false; pic.why = "the slices of a picture refer to different picture parameter sets"; }
                    pic.more.push_back(i);
                    pic.nal_bytes += s.nal_size;
                    continue;
                }
            } else {
                idr.why = "slice refers to a parameter set that was not (successfully) received";
            }
            idrs.push_back(idr);
        }
    }
    if (spec)
        for (Idr &pic : idrs)
            if (pic.ok && !slice_can_hold_picture(pic.sps, pic.nal_bytes)) {
                pic.ok = false;
                pic.why = "the slices of the picture are too small, together, for the picture size of its SPS";
            }
    return RC_SUCCESS;
}

// MP4: parameter sets come from the avcC box, pictures from the sync samples of the first
// video track; a sample is a sequence of length-prefixed NAL units.  The decode target is "the same pictures as the
// elementary-stream path" -- in-band SPS/PPS are honoured, the first IDR slice NAL of a sync sample is the picture.
int mvhp_stream::build_mp4(std::string &err)
{
    mp4::VideoTrack trk;
    if (!mp4::parse(data, size, trk, err)) return RC_FAILURE;
    quarter_turns = trk.quarter_turns;
    Sps sps_tab[32];
    Pps pps_tab[256];
    std::vector<uint8_t> rbsp;
    auto add_param = [&](size_t off, size_t len) {
        if (len < 2 || off + len > size) return;
        const int type = data[off] & 31;
        unescape_rbsp(data + off + 1, len - 1, rbsp);
        BitReader br(rbsp.data(), rbsp.size());
        std::string e;
        if (type == 7) { Sps sps; if (parse_sps(br, sps, e) == RC_SUCCESS) sps_tab[sps.sps_id] = sps; else param_errors++; }
        else if (type == 8) { Pps pps; if (parse_pps(br, sps_tab, pps, e) == RC_SUCCESS) pps_tab[pps.pps_id] = pps; else param_errors++; }
    };
    for (const mp4::NalRef &n : trk.sps) add_param(n.offset, n.size);
    for (const mp4::NalRef &n : trk.pps) add_param(n.offset, n.size);
    for (const mp4::Sample &smp : trk.samples) {
        if (!smp.sync || smp.size == 0) continue;
        size_t p = smp.offset;
        const size_t end = smp.offset + smp.size;
        bool took = false;
        while (p + (size_t)trk.nal_length_size < end) {
            size_t len = 0;
            for (int i = 0; i < trk.nal_length_size; i++) len = (len << 8) | data[p + i];
            p += (size_t)trk.nal_length_size;
            if (len == 0 || len > end - p) break;
            const int type = data[p] & 31;
            if (type == 7 || type == 8) add_param(p, len);
            else if (type == 5 && !took) {
                EsSample s;
                s.offset = p;
                s.sample_size = s.nal_size = len;
                s.nal_unit_type = 5;
                s.nal_ref_idc = (data[p] >> 5) & 3;
                s.is_idr = true;
                samples.push_back(s);
                Idr idr;
                idr.sample = samples.size() - 1;
                unescape_rbsp(data + p + 1, len - 1 < 16 ? len - 1 : 16, rbsp);
                BitReader br(rbsp.data(), rbsp.size());
                br.ue();
                br.ue();
                const unsigned pid = br.ue();
                if (pid < 256 && pps_tab[pid].valid && sps_tab[pps_tab[pid].sps_id].valid) {
                    idr.pps = pps_tab[pid];
                    idr.sps = sps_tab[idr.pps.sps_id];
                    idr.ok = slice_can_hold_picture(idr.sps, len);
                    if (!idr.ok) idr.why = "slice NAL too small for the picture size of its SPS";
                } else {
                    idr.why = "slice refers to a parameter set that was not (successfully) received";
                }
                idrs.push_back(idr);
                took = true;
            }
            p += len;
        }
    }
    if (idrs.empty()) { err = "MP4: no IDR picture in the sync samples"; return RC_FAILURE; }
    return RC_SUCCESS;
}

// the slice NAL units of picture `idr`, unescaped: one in the reference's world, several for MVHP_STREAM_SPEC streams
static void picture_slices(const mvhp_stream &st, const mvhp_stream::Idr &idr, std::vector<std::vector<uint8_t>> &store,
                           std::vector<SliceRbsp> &slices)
{
    store.resize(1 + idr.more.size());
    slices.resize(store.size());
    for (size_t k = 0; k < store.size(); k++) {
        const EsSample &s = st.samples[k == 0 ? idr.sample : idr.more[k - 1]];
        unescape_rbsp(st.data + s.offset + 1, s.nal_size - 1, store[k]);
        slices[k].rbsp = store[k].data();
        slices[k].n = store[k].size();
        slices[k].nal_ref_idc = s.nal_ref_idc;
    }
}

int mvhp_stream::decode_packed(int k, void *packed, size_t bytes, std::string &err) const
{
    if (k < 0 || (size_t)k >= idrs.size()) { err = "IDR index out of range"; return RC_FAILURE; }
    const Idr &idr = idrs[k];
    if (!idr.ok) { err = idr.why; return RC_FAILURE; }
    std::vector<std::vector<uint8_t>> store;
    std::vector<SliceRbsp> slices;
    picture_slices(*this, idr, store, slices);
    PictureDecoder pd(idr.sps, idr.pps, slices[0].nal_ref_idc, spec, deblock);
    return pd.decode_slices(slices.data(), (int)slices.size(), (uint8_t *)packed, bytes, err);
}

int mvhp_stream::decode_compact(int k, void *buf, size_t cap, size_t *used, std::string &err) const
{
    if (used) *used = 0;
    if (k < 0 || (size_t)k >= idrs.size()) { err = "IDR index out of range"; return RC_FAILURE; }
    const Idr &idr = idrs[k];
    if (!idr.ok) { err = idr.why; return RC_FAILURE; }
    std::vector<std::vector<uint8_t>> store;
    std::vector<SliceRbsp> slices;
    picture_slices(*this, idr, store, slices);
    PictureDecoder pd(idr.sps, idr.pps, slices[0].nal_ref_idc, spec, deblock);
    return pd.decode_slices_compact(slices.data(), (int)slices.size(), (uint8_t *)buf, cap, used, err);
}

static thread_local std::string g_stream_err;

extern "C" {

MVHP_EXPORT const char *mvhp_stream_last_error(void) { return g_stream_err.c_str(); }

MVHP_EXPORT int mvhp_stream_open(const uint8_t *data, size_t size, mvhp_stream_t **out)
{
    if (!out || !data) return MVHP_FAILURE;
    *out = nullptr;
    mvhp_stream *s = new mvhp_stream();
    s->data = data;
    s->size = size;
    if (s->build(g_stream_err) != RC_SUCCESS) { delete s; return MVHP_FAILURE; }
    *out = s;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_stream_open_ex(const uint8_t *data, size_t size, uint32_t flags, mvhp_stream_t **out)
{
    if (!out || !data || (flags & ~(MVHP_STREAM_SPEC | MVHP_STREAM_DEBLOCK))) return MVHP_FAILURE;
    *out = nullptr;
    mvhp_stream *s = new mvhp_stream();
    s->data = data;
    s->size = size;
    s->spec = (flags & MVHP_STREAM_SPEC) != 0;
    s->deblock = (flags & MVHP_STREAM_DEBLOCK) != 0;
    if (s->build(g_stream_err) != RC_SUCCESS) { delete s; return MVHP_FAILURE; }
    *out = s;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_stream_open_mp4(const uint8_t *data, size_t size, mvhp_stream_t **out)
{
    if (!out || !data) return MVHP_FAILURE;
    *out = nullptr;
    mvhp_stream *s = new mvhp_stream();
    s->data = data;
    s->size = size;
    if (s->build_mp4(g_stream_err) != RC_SUCCESS) { delete s; return MVHP_FAILURE; }
    *out = s;
    return MVHP_SUCCESS;
}

MVHP_EXPORT void mvhp_stream_close(mvhp_stream_t *s) { delete s; }

MVHP_EXPORT int mvhp_stream_idr_count(const mvhp_stream_t *s) { return s ? (int)s->idrs.size() : 0; }

MVHP_EXPORT int mvhp_stream_rotation(const mvhp_stream_t *s) { return s ? 90 * (s->quarter_turns & 3) : 0; }

MVHP_EXPORT int mvhp_stream_display(const mvhp_stream_t *s, int idr, mvhp_display_info_t *out)
{
    if (!s || !out || idr < 0 || (size_t)idr >= s->idrs.size() || !s->idrs[idr].ok) return MVHP_FAILURE;
    const Sps &sps = s->idrs[idr].sps;
    memset(out, 0, sizeof(*out));
    out->sar_w = sps.sar_w;
    out->sar_h = sps.sar_h;
    out->vui_present = sps.vui_present;
    out->signal_present = sps.signal_present;
    out->full_range = sps.full_range;
    out->matrix_coefficients = (uint32_t)sps.matrix_coefficients;
    out->chroma_loc = (uint32_t)sps.chroma_loc;
    return MVHP_SUCCESS;
}

// ---- colour parameters (host only; include/minivideo_hotpath.h "Colour conversion") ----

// round(2^14 num / den), num and den positive
static int32_t q14(__int128 num, __int128 den) { return (int32_t)((2 * num * 16384 + den) / (2 * den)); }

MVHP_EXPORT int mvhp_color_coefficients(int matrix, int full_range, int32_t out[6])
{
    if (!out || (matrix != MVHP_MATRIX_BT601 && matrix != MVHP_MATRIX_BT709) || (full_range != 0 && full_range != 1)) return MVHP_FAILURE;
    // Kr, Kb in ten-thousandths; Kg = 1 - Kr - Kb.  R = Y + 2 (1 - Kr) Cr, B = Y + 2 (1 - Kb) Cb,
    // G = Y - 2 Kb (1 - Kb) / Kg Cb - 2 Kr (1 - Kr) / Kg Cr; limited range scales luma by 255/219 and chroma by 255/224
    const int64_t D = 10000, kr = matrix == MVHP_MATRIX_BT709 ? 2126 : 2990, kb = matrix == MVHP_MATRIX_BT709 ? 722 : 1140;
    const int64_t kg = D - kr - kb;
    const int64_t ln = full_range ? 1 : 255, ld = full_range ? 1 : 219, cn = full_range ? 1 : 255, cd = full_range ? 1 : 224;
    out[0] = q14(ln, ld);
    out[1] = q14((__int128)2 * (D - kr) * cn, (__int128)D * cd);
    out[2] = q14((__int128)2 * (D - kb) * cn, (__int128)D * cd);
    out[3] = q14((__int128)2 * kb * (D - kb) * cn, (__int128)kg * D * cd);
    out[4] = q14((__int128)2 * kr * (D - kr) * cn, (__int128)kg * D * cd);
    out[5] = full_range ? 0 : 16;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_color_resolve(const mvhp_display_info_t *d, uint32_t coded_w, uint32_t coded_h, int mode, mvhp_color_params_t *out)
{
    if (!out || mode < 0 || mode > 4) return MVHP_FAILURE;
    memset(out, 0, sizeof(*out));
    if (mode == 0) {
        const uint32_t mc = d ? d->matrix_coefficients : 2u;
        if (mc == 1) out->matrix = MVHP_MATRIX_BT709;
        else if (mc == 5 || mc == 6) out->matrix = MVHP_MATRIX_BT601;
        else out->matrix = (coded_w >= 1280 || coded_h > 576) ? MVHP_MATRIX_BT709 : MVHP_MATRIX_BT601;   // unspecified or unsupported
        out->full_range = d && d->signal_present && d->full_range;
    } else {
        out->matrix = (mode == 2 || mode == 4) ? MVHP_MATRIX_BT709 : MVHP_MATRIX_BT601;
        out->full_range = mode >= 3;
    }
    out->siting = (d && (d->chroma_loc & 1)) ? MVHP_CHROMA_CENTER : MVHP_CHROMA_LEFT;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_stream_params(const mvhp_stream_t *s, int idr, mvhp_stream_params_t *out)
{
    if (!s || !out || idr < 0 || (size_t)idr >= s->idrs.size() || !s->idrs[idr].ok) return MVHP_FAILURE;
    const mvhp_stream::Idr &i = s->idrs[idr];
    out->width_mbs = (uint32_t)i.sps.width_mbs;
    out->height_mbs = (uint32_t)i.sps.height_map_units;
    out->chroma_qp_index_offset = i.pps.chroma_qp_index_offset;
    out->second_chroma_qp_index_offset = i.pps.second_chroma_qp_index_offset;
    out->flags = (i.pps.transform_8x8_mode ? MVHP_PARAM_MAY_HAVE_8X8 : 0u) | (s->spec ? MVHP_PARAM_SPEC_LUMA_DC : 0u) |
                 (s->deblock ? MVHP_PARAM_DEBLOCK : 0u);
    memset(out->scaling4, 16, sizeof(out->scaling4));
    memset(out->scaling8, 16, sizeof(out->scaling8));
    if (s->spec) {   // SURVEY 8f row f4 (outside parity): several slices, scaling matrices
        if (!i.more.empty()) out->flags |= MVHP_PARAM_SLICES;
        if ((i.sps.scaling.present || i.pps.scaling.present) &&
            effective_intra_scaling(i.sps.scaling, i.pps.scaling, i.pps.transform_8x8_mode, out->scaling4, out->scaling8))
            out->flags |= MVHP_PARAM_SCALING;
    }
    return MVHP_SUCCESS;
}

// The SPS cropping rectangle (7.4.2.1.1; frame macroblocks, 4:2:0: CropUnitX = CropUnitY = 2).  The reference derives the
// same (h264_parameterset.c:360-378) and never applies it; nothing here changes what a picture decodes to.
MVHP_EXPORT int mvhp_stream_crop(const mvhp_stream_t *s, int idr, mvhp_output_geometry_t *out)
{
    if (!s || !out || idr < 0 || (size_t)idr >= s->idrs.size() || !s->idrs[idr].ok) {
        g_stream_err = "mvhp_stream_crop: no parameter sets for this picture";
        return MVHP_FAILURE;
    }
    const Sps &sps = s->idrs[idr].sps;
    const int64_t W = (int64_t)sps.width_mbs * 16, H = (int64_t)sps.height_map_units * 16;
    int64_t c[4] = {0, 0, 0, 0};   // left, right, top, bottom (frame_crop_*_offset)
    if (sps.frame_cropping)
        for (int i = 0; i < 4; i++) c[i] = (int64_t)(uint32_t)sps.crop[i];
    const int64_t w = W - 2 * (c[0] + c[1]), h = H - 2 * (c[2] + c[3]);
    if (w <= 0 || h <= 0) {
        g_stream_err = "SPS frame cropping leaves no picture (" + std::to_string(W) + "x" + std::to_string(H) + " coded, offsets " +
                       std::to_string(c[0]) + " " + std::to_string(c[1]) + " " + std::to_string(c[2]) + " " + std::to_string(c[3]) + ")";
        return MVHP_FAILURE;
    }
    memset(out, 0, sizeof(*out));
    out->crop_x = (uint32_t)(2 * c[0]);
    out->crop_y = (uint32_t)(2 * c[2]);
    out->crop_w = out->out_w = (uint32_t)w;
    out->crop_h = out->out_h = (uint32_t)h;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_geometry_fit(uint32_t cw, uint32_t ch, uint32_t bw, uint32_t bh, uint32_t *ow, uint32_t *oh)
{
    uint32_t w = 0, h = 0;
    if (!ow || !oh || (cw & 1) || (ch & 1) || !mvrs::fit(cw, ch, bw, bh, w, h)) return MVHP_FAILURE;
    *ow = w;
    *oh = h;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_geometry_aspect(uint32_t cw, uint32_t ch, uint32_t sar_w, uint32_t sar_h, uint32_t *ow, uint32_t *oh)
{
    uint32_t w = 0, h = 0;
    if (!ow || !oh || (cw & 1) || (ch & 1) || !mvrs::aspect(cw, ch, sar_w, sar_h, w, h)) return MVHP_FAILURE;
    *ow = w;
    *oh = h;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_output_turns(const mvhp_stream_t *s, const mvhp_output_request_t *req)
{
    if (!req) return 0;
    const int own = (s && (req->flags & MVHP_OUTPUT_ORIENT)) ? s->quarter_turns : 0;
    return (own + (int)((req->flags & MVHP_OUTPUT_ROTATE_MASK) >> MVHP_OUTPUT_ROTATE_SHIFT)) & 3;
}

MVHP_EXPORT int mvhp_output_geometry(const mvhp_stream_t *s, int idr, const mvhp_output_request_t *req_in, mvhp_output_geometry_t *out)
{
    // the turn: the geometry is formed in the coded picture's orientation -- for odd turns against the box turned back -- and the
    // sides of the output are exchanged afterwards; crop_* stay coded coordinates.  Zero turns: the request without these bits
    const int turns = mvhp_output_turns(s, req_in);
    mvhp_output_request_t unturned;
    const mvhp_output_request_t *req = req_in;
    if (req_in && (req_in->flags & (MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE_MASK))) {   // colour changes no geometry
        mvhp_output_request_t plain = *req_in;
        plain.flags &= ~(MVHP_OUTPUT_COLOR | MVHP_OUTPUT_COLOR_MODE_MASK);
        return mvhp_output_geometry(s, idr, &plain, out);
    }
    if (req_in && (req_in->flags & (MVHP_OUTPUT_ORIENT | MVHP_OUTPUT_ROTATE_MASK))) {
        unturned = *req_in;
        unturned.flags &= ~(MVHP_OUTPUT_ORIENT | MVHP_OUTPUT_ROTATE_MASK);
        if (turns & 1) std::swap(unturned.box_w, unturned.box_h);
        req = &unturned;
        if (out && (turns & 1)) {
            const int rc = mvhp_output_geometry(s, idr, req, out);
            if (rc == MVHP_SUCCESS) std::swap(out->out_w, out->out_h);
            return rc;
        }
    }
    if (!req || req->flags == 0) {   // the coded size
        mvhp_stream_params_t p;
        if (!out || mvhp_stream_params(s, idr, &p) != MVHP_SUCCESS) {
            g_stream_err = "mvhp_output_geometry: no parameter sets for this picture";
            return MVHP_FAILURE;
        }
        memset(out, 0, sizeof(*out));
        out->crop_w = out->out_w = p.width_mbs * 16;
        out->crop_h = out->out_h = p.height_mbs * 16;
        return MVHP_SUCCESS;
    }
    if ((req->flags & ~(MVHP_OUTPUT_CROP | MVHP_OUTPUT_BOX | MVHP_OUTPUT_ASPECT | MVHP_OUTPUT_TRIM)) || ((req->flags & MVHP_OUTPUT_BOX) && (req->box_w < 2 || req->box_h < 2))) {
        g_stream_err = "mvhp_output_geometry: malformed request (box sides must be at least 2)";
        return MVHP_FAILURE;
    }
    if (mvhp_stream_crop(s, idr, out) != MVHP_SUCCESS) return MVHP_FAILURE;
    if ((req->flags & MVHP_OUTPUT_TRIM) && s->trim[2] && s->trim[3]) {   // black bars: the stream's box, where the rule trusts it
        mvhp_luma_bars_t u{};
        u.x = s->trim[0]; u.y = s->trim[1]; u.w = s->trim[2]; u.h = s->trim[3];
        mvbars::trim_rect(*out, &u, *out);   // (0: this picture keeps its SPS crop)
    }
    if (req->flags & MVHP_OUTPUT_ASPECT) {   // square samples first: one axis of the crop shrinks; the box is fitted to that size
        const Sps &sps = s->idrs[idr].sps;
        mvrs::aspect(out->crop_w, out->crop_h, sps.sar_w, sps.sar_h, out->out_w, out->out_h);
    }
    if (req->flags & MVHP_OUTPUT_BOX) {
        const uint32_t dw = out->out_w, dh = out->out_h;
        mvrs::fit(dw, dh, req->box_w, req->box_h, out->out_w, out->out_h);
    }
    return MVHP_SUCCESS;
}

// ---- black bars (host only; include/minivideo_hotpath.h "Black bars") ----

MVHP_EXPORT uint32_t mvhp_bars_need(uint32_t len) { return mvbars::need(len); }

MVHP_EXPORT int mvhp_bars_union(const mvhp_luma_bars_t *b, int n, mvhp_luma_bars_t *out)
{
    mvhp_luma_bars_t u;
    const int found = mvbars::unite(b, n, u);
    if (out) *out = u;
    return found;
}

MVHP_EXPORT int mvhp_trim_rect(const mvhp_output_geometry_t *crop, const mvhp_luma_bars_t *u, mvhp_output_geometry_t *out)
{
    if (!crop || !out) return 0;
    const mvhp_output_geometry_t c = *crop;
    return mvbars::trim_rect(c, u, *out);
}

MVHP_EXPORT int mvhp_stream_set_trim(mvhp_stream_t *s, const mvhp_luma_bars_t *u)
{
    if (!s) return MVHP_FAILURE;
    const bool none = !u || mvbars::empty(*u);
    s->trim[0] = none ? 0 : u->x; s->trim[1] = none ? 0 : u->y;
    s->trim[2] = none ? 0 : u->w; s->trim[3] = none ? 0 : u->h;
    return MVHP_SUCCESS;
}

MVHP_EXPORT int mvhp_stream_trim(const mvhp_stream_t *s, mvhp_luma_bars_t *out)
{
    if (!s || !out) return MVHP_FAILURE;
    memset(out, 0, sizeof(*out));
    out->x = s->trim[0]; out->y = s->trim[1]; out->w = s->trim[2]; out->h = s->trim[3];
    return MVHP_SUCCESS;
}

MVHP_EXPORT size_t mvhp_geometry_yuv_bytes(const mvhp_output_geometry_t *g)
{
    return g ? (size_t)g->out_w * g->out_h * 3 / 2 : 0;
}

MVHP_EXPORT size_t mvhp_geometry_rgb_bytes(const mvhp_output_geometry_t *g)
{
    return g ? (size_t)g->out_w * g->out_h * 3 : 0;
}

MVHP_EXPORT size_t mvhp_tensor_bytes(const mvhp_tensor_params_t *t) { return t ? mvtensor::bytes(*t) : 0; }

MVHP_EXPORT int mvhp_tensor_constants(const double mean[3], const double std[3], float scale[3], float bias[3])
{
    return mvtensor::constants(mean, std, scale, bias) ? MVHP_SUCCESS : MVHP_FAILURE;
}

MVHP_EXPORT int mvhp_stream_decode_packed(const mvhp_stream_t *s, int idr, void *packed, size_t packed_bytes)
{
    if (!s || !packed) return MVHP_FAILURE;
    std::string err;
    const int rc = s->decode_packed(idr, packed, packed_bytes, err);
    if (rc != RC_SUCCESS) g_stream_err = err;
    return rc;
}

MVHP_EXPORT int mvhp_stream_decode_compact(const mvhp_stream_t *s, int idr, void *buf, size_t cap, size_t *used)
{
    if (!s || !buf) return MVHP_FAILURE;
    std::string err;
    const int rc = s->decode_compact(idr, buf, cap, used, err);
    if (rc != RC_SUCCESS) g_stream_err = err;
    return rc;
}

} // extern "C"
