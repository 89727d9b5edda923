// tensor_policy.h -- tensor output (opt-in; DESIGN.md 3 "Tensor output"): what is a well-formed set of tensor parameters, how many
// bytes a picture's tensor has, and the normalisation constants.  Host arithmetic only, shared by the C-ABI (stream_abi.cpp,
// hotpath_abi.hip), the engine and its CPU harness.
#pragma once
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "minivideo_hotpath.h"

namespace mvtensor {

constexpr uint32_t kMaxSide = 16384;

inline size_t element_bytes(uint32_t dtype) { return dtype == MVHP_TENSOR_F32 ? 4 : 2; }

// what is wrong with the parameters, in the words of the field (nullptr: nothing); scale / bias are judged by finite()
inline const char *malformed(const mvhp_tensor_params_t &t)
{
    if (t.dtype > MVHP_TENSOR_BF16) return "dtype";
    if (t.layout > MVHP_TENSOR_NHWC) return "layout";
    if (t.flags & ~MVHP_TENSOR_BGR) return "flags";
    if (t.src_w < 1 || t.src_w > kMaxSide) return "src_w";
    if (t.src_h < 1 || t.src_h > kMaxSide) return "src_h";
    if ((t.canvas_w == 0) != (t.canvas_h == 0)) return "canvas_w, canvas_h (both 0 or neither)";
    if (t.canvas_w && (t.canvas_w < t.src_w || t.canvas_w > kMaxSide)) return "canvas_w";
    if (t.canvas_h && (t.canvas_h < t.src_h || t.canvas_h > kMaxSide)) return "canvas_h";
    return nullptr;
}

inline bool finite(const mvhp_tensor_params_t &t)
{
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(t.scale[k]) || !std::isfinite(t.bias[k])) return false;
    return true;
}

inline uint32_t canvas_w(const mvhp_tensor_params_t &t) { return t.canvas_w ? t.canvas_w : t.src_w; }
inline uint32_t canvas_h(const mvhp_tensor_params_t &t) { return t.canvas_h ? t.canvas_h : t.src_h; }

inline size_t bytes(const mvhp_tensor_params_t &t)
{
    if (malformed(t)) return 0;
    return (size_t)3 * canvas_w(t) * canvas_h(t) * element_bytes(t.dtype);
}

inline bool constants(const double mean[3], const double sd[3], float scale[3], float bias[3])
{
    if (!mean || !sd || !scale || !bias) return false;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(mean[k]) || !std::isfinite(sd[k]) || sd[k] == 0.0) return false;
    for (int k = 0; k < 3; k++) {
        scale[k] = (float)(1.0 / (255.0 * sd[k]));
        bias[k] = (float)(-mean[k] / sd[k]);
    }
    return true;
}

// the parameters of a picture of src_w x src_h under an engine request
inline mvhp_tensor_params_t of_request(const mvhp_tensor_request_t &r, uint32_t src_w, uint32_t src_h)
{
    mvhp_tensor_params_t t{};
    t.src_w = src_w; t.src_h = src_h;
    t.canvas_w = r.canvas_w; t.canvas_h = r.canvas_h;
    t.dtype = r.dtype; t.layout = r.layout; t.flags = r.flags; t.pad_rgb = r.pad_rgb;
    for (int k = 0; k < 3; k++) { t.scale[k] = r.scale[k]; t.bias[k] = r.bias[k]; }
    return t;
}

} // namespace mvtensor
