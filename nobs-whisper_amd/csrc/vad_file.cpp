// The Silero-VAD model file (ggml's legacy container, as tools/make_vad_model.py writes it; vad_segments.h). No HIP
// header. The layout restates whisper.cpp's converter from memory and is unverified against a real file.
#include <cstdio>
#include <cstring>

#include "vad_segments.h"

namespace wm {
namespace {

struct Reader {
    const uint8_t* p;
    size_t left;
    bool take(void* dst, size_t n) {
        if (n > left) return false;
        if (n) memcpy(dst, p, n);
        p += n;
        left -= n;
        return true;
    }
    bool i32(int32_t& v) { return take(&v, 4); }
};

float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1f, mant = h & 0x3ffu, x;
    if (exp == 0) {
        if (mant == 0) x = sign;
        else {
            int e = -1;
            do { e++; mant <<= 1; } while (!(mant & 0x400u));
            mant &= 0x3ffu;
            x = sign | ((uint32_t)(127 - 15 - e) << 23) | (mant << 13);
        }
    } else if (exp == 0x1f) x = sign | 0x7f800000u | (mant << 13);
    else x = sign | ((exp + 127 - 15) << 23) | (mant << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

struct Want { std::string name; std::vector<int> shape; std::vector<float>* dst; bool seen; };

bool refuse(std::string* err, const std::string& why) {
    if (err) *err = why;
    return false;
}

}  // namespace

bool vad_parse(const uint8_t* data, size_t size, VadFile& out, std::string* err) {
    Reader r{data, size};
    uint32_t magic = 0;
    if (!r.take(&magic, 4)) return refuse(err, "truncated header");
    if (magic != 0x67676d6cu) return refuse(err, "bad magic");
    int32_t len = 0;
    if (!r.i32(len)) return refuse(err, "truncated header");
    if (len < 0 || len > 64 || (size_t)len > r.left) return refuse(err, "bad model-type string");
    std::string type((const char*)r.p, (size_t)len);
    r.p += len;
    r.left -= len;
    if (type != "silero-16k") return refuse(err, "model type '" + type + "' is not silero-16k");
    int32_t ver[3], n_layers = 0;
    for (int32_t& v : ver)
        if (!r.i32(v)) return refuse(err, "truncated header");
    if (ver[0] != 5) return refuse(err, "version " + std::to_string(ver[0]) + " is not 5");
    if (!r.i32(n_layers)) return refuse(err, "truncated header");
    if (n_layers != 4) return refuse(err, "n_encoder_layers is not 4");
    for (int l = 0; l < 4; l++) {
        int32_t g[3];
        for (int32_t& v : g)
            if (!r.i32(v)) return refuse(err, "truncated header");
        if (g[0] != kVadConvIn[l] || g[1] != kVadConvOut[l] || g[2] != 3) return refuse(err, "encoder layer " + std::to_string(l) + " has another geometry");
    }
    int32_t tail[4];
    for (int32_t& v : tail)
        if (!r.i32(v)) return refuse(err, "truncated header");
    if (tail[0] != kVadHidden || tail[1] != kVadHidden || tail[2] != kVadHidden || tail[3] != 1) return refuse(err, "LSTM / head geometry is not 128, 128, 128, 1");

    std::vector<Want> want;
    want.push_back({"_model.stft.forward_basis_buffer", {2 * kVadBins, 1, kVadFft}, &out.basis, false});
    for (int l = 0; l < 4; l++) {
        const std::string pre = "_model.encoder." + std::to_string(l) + ".reparam_conv.";
        want.push_back({pre + "weight", {kVadConvOut[l], kVadConvIn[l], 3}, &out.conv_w[l], false});
        want.push_back({pre + "bias", {kVadConvOut[l]}, &out.conv_b[l], false});
    }
    want.push_back({"_model.decoder.rnn.weight_ih", {4 * kVadHidden, kVadHidden}, &out.w_ih, false});
    want.push_back({"_model.decoder.rnn.weight_hh", {4 * kVadHidden, kVadHidden}, &out.w_hh, false});
    want.push_back({"_model.decoder.rnn.bias_ih", {4 * kVadHidden}, &out.b_ih, false});
    want.push_back({"_model.decoder.rnn.bias_hh", {4 * kVadHidden}, &out.b_hh, false});
    want.push_back({"_model.decoder.decoder.2.weight", {1, kVadHidden, 1}, &out.head_w, false});
    want.push_back({"_model.decoder.decoder.2.bias", {1}, &out.head_b, false});

    while (r.left > 0) {
        int32_t n_dims = 0, name_len = 0, ftype = 0;
        if (!r.i32(n_dims) || !r.i32(name_len) || !r.i32(ftype)) return refuse(err, "truncated tensor record");
        if (n_dims < 1 || n_dims > 4 || name_len < 1 || name_len > 256) return refuse(err, "bad tensor record");
        if (ftype != 0 && ftype != 1) return refuse(err, "tensor element type " + std::to_string(ftype) + " is neither f32 nor f16");
        int32_t ne[4];
        for (int d = 0; d < n_dims; d++)
            if (!r.i32(ne[d])) return refuse(err, "truncated tensor record");
        if ((size_t)name_len > r.left) return refuse(err, "truncated tensor record");
        const std::string name((const char*)r.p, (size_t)name_len);
        r.p += name_len;
        r.left -= name_len;
        Want* w = nullptr;
        for (Want& q : want)
            if (q.name == name) w = &q;
        if (!w) return refuse(err, "unknown tensor '" + name + "'");
        if (w->seen) return refuse(err, "duplicate tensor '" + name + "'");
        bool same = (int)w->shape.size() == n_dims;
        size_t count = 1;
        for (int d = 0; same && d < n_dims; d++) {  // ggml order: the torch shape reversed
            same = ne[d] == w->shape[n_dims - 1 - d];
            count *= (size_t)w->shape[n_dims - 1 - d];
        }
        if (!same) return refuse(err, "tensor '" + name + "' has another shape");
        const size_t bytes = count * (ftype == 0 ? 4 : 2);
        if (bytes > r.left) return refuse(err, "truncated data of tensor '" + name + "'");
        w->dst->resize(count);
        if (ftype == 0) memcpy(w->dst->data(), r.p, bytes);
        else
            for (size_t i = 0; i < count; i++) {
                uint16_t h;
                memcpy(&h, r.p + 2 * i, 2);
                (*w->dst)[i] = half_to_float(h);
            }
        r.p += bytes;
        r.left -= bytes;
        w->seen = true;
    }
    for (const Want& q : want)
        if (!q.seen) return refuse(err, "missing tensor '" + q.name + "'");
    return true;
}

}  // namespace wm
