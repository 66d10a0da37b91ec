// Silero-VAD on the device: the model's upload and the two runs (probabilities, filtered PCM) over kernels/vad.hip
// (vad.h).
#include "vad.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "common.h"

namespace wm {

namespace {
template <typename T> void grow(T*& p, size_t& cap, size_t need) {
    if (cap >= need) return;
    if (p) WM_CHECK(hipFree(p));
    p = nullptr;
    cap = 0;
    WM_CHECK(hipMalloc((void**)&p, std::max<size_t>(need, 64) * sizeof(T)));
    cap = std::max<size_t>(need, 64);
}
template <typename T> void grow(T*& p, int& cap, size_t need) {
    size_t c = (size_t)cap;
    grow(p, c, need);
    cap = (int)c;
}
inline size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

struct Timed {
    const VadHooks* h;
    Timed(const VadHooks* h_, int kernel, double bytes) : h(h_) { if (h) h->begin(h->u, kernel, bytes); }
    ~Timed() { if (h) h->end(h->u); }
};
}  // namespace

VadModel* vad_model_load(const uint8_t* data, size_t size, int device, std::string* err) {
    VadFile f;
    if (!vad_parse(data, size, f, err)) return nullptr;
    // one host image in the kernels' layouts (vad.h), every part on a 64-float boundary
    std::vector<float> img;
    const auto put = [&](const std::vector<float>& v) {
        const size_t at = img.size();
        img.insert(img.end(), v.begin(), v.end());
        img.resize(align64(img.size()), 0.0f);
        return at;
    };
    std::vector<float> t((size_t)kVadFft * 2 * kVadBins);
    for (int r = 0; r < 2 * kVadBins; r++)
        for (int k = 0; k < kVadFft; k++) t[(size_t)k * 2 * kVadBins + r] = f.basis[(size_t)r * kVadFft + k];
    const size_t o_basis = put(t);
    size_t o_cw[4], o_cb[4];
    for (int l = 0; l < 4; l++) {
        const int ci = kVadConvIn[l], co = kVadConvOut[l], cp = l == 0 ? kVadC0Pad : ci;
        t.assign((size_t)3 * cp * co, 0.0f);
        for (int o = 0; o < co; o++)
            for (int c = 0; c < ci; c++)
                for (int tap = 0; tap < 3; tap++) t[((size_t)tap * cp + c) * co + o] = f.conv_w[l][((size_t)o * ci + c) * 3 + tap];
        o_cw[l] = put(t);
        o_cb[l] = put(f.conv_b[l]);
    }
    t.assign((size_t)kVadHidden * 4 * kVadHidden, 0.0f);
    for (int o = 0; o < 4 * kVadHidden; o++)
        for (int k = 0; k < kVadHidden; k++) t[(size_t)k * 4 * kVadHidden + o] = f.w_ih[(size_t)o * kVadHidden + k];
    const size_t o_wih = put(t), o_bih = put(f.b_ih), o_bhh = put(f.b_hh), o_whh = put(f.w_hh), o_hw = put(f.head_w);

    VadModel* m = new VadModel();
    m->device = device;
    try {
        WM_CHECK(hipSetDevice(device));
        WM_CHECK(hipMalloc((void**)&m->blob, img.size() * sizeof(float)));
        WM_CHECK(hipMemcpy(m->blob, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    } catch (...) {
        if (m->blob) hipFree(m->blob);
        delete m;
        throw;
    }
    VadWeights& w = m->w;
    w.basis_t = m->blob + o_basis;
    for (int l = 0; l < 4; l++) { w.conv_t[l] = m->blob + o_cw[l]; w.conv_b[l] = m->blob + o_cb[l]; }
    w.wih_t = m->blob + o_wih;
    w.b_ih = m->blob + o_bih;
    w.b_hh = m->blob + o_bhh;
    w.whh = m->blob + o_whh;
    w.head_w = m->blob + o_hw;
    w.head_b = f.head_b[0];
    return m;
}

VadModel* vad_model_load_file(const char* path, int device, std::string* err) {
    FILE* fp = path ? fopen(path, "rb") : nullptr;
    if (!fp) {
        if (err) *err = path ? "cannot open the file" : "no model path";
        return nullptr;
    }
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, fp)) > 0) {
        buf.insert(buf.end(), chunk, chunk + n);
        if (buf.size() > ((size_t)64 << 20)) break;  // (a VAD model is about 1 MB)
    }
    fclose(fp);
    return vad_model_load(buf.data(), buf.size(), device, err);
}

void vad_model_free(VadModel* m) {
    if (!m) return;
    if (m->blob) hipFree(m->blob);
    delete m;
}

void vad_scratch_free(VadScratch& sc) {
    for (void* p : {(void*)sc.pcm, (void*)sc.xg, (void*)sc.h, (void*)sc.probs, (void*)sc.out, (void*)sc.clips, (void*)sc.gclips, (void*)sc.pieces})
        if (p) hipFree(p);
    sc = VadScratch();
}

void vad_probs_run(const VadModel& m, VadScratch& sc, const float* const* pcm, const int* n, int n_clips, bool on_device,
                   hipStream_t st, const VadHooks* hooks, std::vector<std::vector<float>>& probs, float* xg_out) {
    probs.assign(n_clips, {});
    sc.dev_pcm.assign(n_clips, nullptr);
    if (n_clips <= 0) return;
    size_t pcm_tot = 0, win_tot = 0;
    int max_win = 0;
    for (int j = 0; j < n_clips; j++) {
        pcm_tot += align64((size_t)n[j]);
        const int nw = (int)(((long long)n[j] + kVadWindow - 1) / kVadWindow);
        win_tot += (size_t)nw;
        max_win = std::max(max_win, nw);
    }
    if (!on_device) grow(sc.pcm, sc.cap_pcm, pcm_tot);
    grow(sc.xg, sc.cap_xg, win_tot * 4 * kVadHidden);
    grow(sc.h, sc.cap_h, win_tot * kVadHidden);
    grow(sc.probs, sc.cap_probs, win_tot);
    grow(sc.clips, sc.cap_clips, (size_t)n_clips);
    std::vector<VadClip> cl(n_clips);
    size_t po = 0;
    long long w0 = 0;
    for (int j = 0; j < n_clips; j++) {
        if (on_device) sc.dev_pcm[j] = pcm[j];
        else {
            sc.dev_pcm[j] = sc.pcm + po;
            if (n[j] > 0) WM_CHECK(hipMemcpyAsync(sc.pcm + po, pcm[j], (size_t)n[j] * 4, hipMemcpyHostToDevice, st));
            po += align64((size_t)n[j]);
        }
        const int nw = (int)(((long long)n[j] + kVadWindow - 1) / kVadWindow);
        cl[j] = VadClip{sc.dev_pcm[j], n[j], nw, w0};
        w0 += nw;
    }
    WM_CHECK(hipMemcpyAsync(sc.clips, cl.data(), cl.size() * sizeof(VadClip), hipMemcpyHostToDevice, st));
    if (win_tot > 0) {
        {
            double bytes = 0;
            for (int j = 0; j < n_clips; j++) bytes += 4.0 * n[j];
            Timed tm(hooks, 0, bytes + (double)win_tot * 4 * kVadHidden * 4);
            launch_vad_frontend(m.w, sc.clips, n_clips, max_win, sc.xg, st);
        }
        {
            Timed tm(hooks, 1, (double)win_tot * (4 * kVadHidden + 2 * kVadHidden + 1) * 4);
            launch_vad_lstm(m.w, sc.clips, n_clips, sc.xg, sc.h, sc.probs, st);
        }
    }
    std::vector<float> all(win_tot);
    if (win_tot > 0) WM_CHECK(hipMemcpyAsync(all.data(), sc.probs, win_tot * 4, hipMemcpyDeviceToHost, st));
    if (xg_out && cl[0].n_win > 0)
        WM_CHECK(hipMemcpyAsync(xg_out, sc.xg, (size_t)cl[0].n_win * 4 * kVadHidden * 4, hipMemcpyDeviceToHost, st));
    WM_CHECK(hipStreamSynchronize(st));  // cl, the caller's PCM (pageable) and `all` must outlive the copies
    for (int j = 0; j < n_clips; j++) probs[j].assign(all.begin() + cl[j].win0, all.begin() + cl[j].win0 + cl[j].n_win);
}

void vad_gather_run(VadScratch& sc, const float* const* dev_pcm, const std::vector<std::vector<VadPiece>>& tables, hipStream_t st,
                    const VadHooks* hooks, std::vector<const float*>& out_ptr, std::vector<int>& out_len) {
    const int n_clips = (int)tables.size();
    out_ptr.assign(n_clips, nullptr);
    out_len.assign(n_clips, 0);
    if (n_clips <= 0) return;
    size_t out_tot = 0, n_pieces = 0;
    int max_out = 0;
    for (const auto& t : tables) {
        out_tot += align64((size_t)vad_filtered_len(t));
        n_pieces += t.size();
        max_out = std::max(max_out, vad_filtered_len(t));
    }
    grow(sc.out, sc.cap_out, out_tot);
    grow(sc.pieces, sc.cap_pieces, n_pieces);
    grow(sc.gclips, sc.cap_gclips, (size_t)n_clips);
    std::vector<VadGatherClip> gc(n_clips);
    std::vector<VadPiece> flat;
    flat.reserve(n_pieces);
    size_t oo = 0;
    for (int j = 0; j < n_clips; j++) {
        out_len[j] = vad_filtered_len(tables[j]);
        out_ptr[j] = sc.out + oo;  // (a clip without speech: length 0, the pointer is never read)
        gc[j] = VadGatherClip{dev_pcm[j], sc.out + oo, (int)flat.size(), (int)tables[j].size(), out_len[j]};
        flat.insert(flat.end(), tables[j].begin(), tables[j].end());
        oo += align64((size_t)out_len[j]);
    }
    WM_CHECK(hipMemcpyAsync(sc.gclips, gc.data(), gc.size() * sizeof(VadGatherClip), hipMemcpyHostToDevice, st));
    if (!flat.empty()) WM_CHECK(hipMemcpyAsync(sc.pieces, flat.data(), flat.size() * sizeof(VadPiece), hipMemcpyHostToDevice, st));
    {
        double bytes = 0;
        for (int j = 0; j < n_clips; j++) bytes += 8.0 * out_len[j];
        Timed tm(hooks, 2, bytes);
        launch_vad_gather(sc.gclips, sc.pieces, n_clips, max_out, st);
    }
    WM_CHECK(hipStreamSynchronize(st));  // gc and flat (pageable) must outlive the copies
}

}  // namespace wm
