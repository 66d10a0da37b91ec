// Host check of the VAD code that needs no HIP (csrc/vad_segments.cpp, csrc/vad_file.cpp) against tests/vad_ref.py
// (tests/test_vad_host.py builds it with plain g++, and again with -fsanitize=address,undefined). Reads from stdin:
//   case <threshold> <min_speech_ms> <min_silence_ms> <max_speech_s> <pad_ms> <overlap> <n_samples> <n_probs> <n_times>
//        then n_probs probabilities and n_times times (10 ms units on the filtered axis); floats as C hex floats
//     -> "segs N" + N lines "start end", "pieces M" + M lines of four, "map" + n_times mapped times
//   load <path>
//     -> "ok <element count>" or "refused: <reason>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "vad_segments.h"

static float next_float() {
    std::string w;
    std::cin >> w;
    return strtof(w.c_str(), nullptr);
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "case") {
            wm::VadParams p;
            p.threshold = next_float();
            std::cin >> p.min_speech_duration_ms >> p.min_silence_duration_ms;
            p.max_speech_duration_s = next_float();
            std::cin >> p.speech_pad_ms;
            p.samples_overlap = next_float();
            int n_samples, n_probs, n_times;
            std::cin >> n_samples >> n_probs >> n_times;
            std::vector<float> probs(n_probs);
            for (float& v : probs) v = next_float();
            std::vector<long long> times(n_times);
            for (auto& t : times) std::cin >> t;
            const auto segs = wm::vad_segments_from_probs(probs.data(), n_probs, p);
            printf("segs %zu\n", segs.size());
            for (const auto& s : segs) printf("%d %d\n", s.start, s.end);
            const auto tab = wm::vad_piece_table(segs, n_samples, p.samples_overlap);
            printf("pieces %zu\n", tab.size());
            for (const auto& q : tab) printf("%d %d %d %d\n", q.orig_start, q.orig_end, q.vad_start, q.vad_end);
            printf("map");
            for (long long t : times) printf(" %lld", (long long)wm::vad_map_time(tab, t));
            printf("\n");
        } else if (cmd == "load") {
            std::string path;
            std::cin >> path;
            std::vector<unsigned char> buf;
            if (FILE* f = fopen(path.c_str(), "rb")) {
                unsigned char chunk[65536];
                size_t n;
                while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
                fclose(f);
            } else {
                printf("refused: cannot open\n");
                continue;
            }
            // an exact-size heap copy: a read past the image is a sanitizer error
            unsigned char* img = (unsigned char*)malloc(buf.size() ? buf.size() : 1);
            std::copy(buf.begin(), buf.end(), img);
            wm::VadFile vf;
            std::string err;
            if (wm::vad_parse(img, buf.size(), vf, &err)) {
                size_t n = vf.basis.size() + vf.w_ih.size() + vf.w_hh.size() + vf.b_ih.size() + vf.b_hh.size() + vf.head_w.size() + vf.head_b.size();
                for (int l = 0; l < 4; l++) n += vf.conv_w[l].size() + vf.conv_b[l].size();
                printf("ok %zu\n", n);
            } else printf("refused: %s\n", err.c_str());
            free(img);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
