// Beam search bookkeeping on the host (beam.h); no HIP in this translation unit (plain C++17).
#include "beam.h"

#include <algorithm>
#include <cstddef>

namespace wm {

std::vector<BeamPick> beam_select(const std::vector<int>& rows, const std::vector<double>& sum_all,
                                  const BeamCand* cands, int K, const std::vector<int>& positions) {
    struct Entry {
        double key;
        int parent, rank;
    };
    std::vector<Entry> pool;
    for (size_t r = 0; r < rows.size(); r++)
        for (int j = 0; j < K; j++) {
            const BeamCand& c = cands[r * K + j];
            if (c.id < 0 || !(c.p > 0.0f)) break;  // candidates come in rank order: the first hole ends the row
            pool.push_back({sum_all[r] + (double)c.plog, rows[r], j});
        }
    std::stable_sort(pool.begin(), pool.end(), [](const Entry& a, const Entry& b) {
        if (a.key != b.key) return a.key > b.key;
        if (a.parent != b.parent) return a.parent < b.parent;
        return a.rank < b.rank;
    });
    std::vector<BeamPick> picks;
    for (size_t i = 0; i < positions.size(); i++) {
        if (i < pool.size()) picks.push_back({positions[i], pool[i].parent, pool[i].rank});
        else picks.push_back({positions[i], -1, -1});
    }
    return picks;
}

std::vector<KvCopy> beam_copies(const std::vector<BeamPick>& picks, std::vector<std::vector<int>>& held,
                                const std::vector<int>& slots) {
    std::vector<KvCopy> copies;
    const std::vector<std::vector<int>> old = held;
    for (const BeamPick& p : picks) {
        if (p.parent < 0 || p.parent == p.beam) continue;
        const std::vector<int>& src = old[p.parent];
        const std::vector<int>& dst = old[p.beam];
        size_t m = 0;
        while (m < src.size() && m < dst.size() && src[m] == dst[m]) m++;
        if (m < src.size()) copies.push_back({slots[p.beam], slots[p.parent], (int)m, (int)src.size(), 0, 0, 0});
        held[p.beam] = src;
    }
    return copies;
}

long beam_schedule(std::vector<KvCopy>& copies, long units_per_row) {
    long off = 0;
    for (KvCopy& c : copies) {
        bool read = false;
        for (const KvCopy& o : copies) read |= o.src_slot == c.dst_slot;
        c.mode = read ? 1 : 0;
        c.pad = 0;
        c.stage_off = 0;
        if (read) {
            c.stage_off = off;
            off += (long)(c.row1 - c.row0) * units_per_row;
        }
    }
    return off;
}

int beam_winner(const std::vector<double>& score, const std::vector<char>& failed) {
    int best = -1;
    for (size_t b = 0; b < score.size(); b++) {
        if (failed[b]) continue;
        if (best < 0 || score[b] > score[best]) best = (int)b;
    }
    return best;
}

}  // namespace wm
