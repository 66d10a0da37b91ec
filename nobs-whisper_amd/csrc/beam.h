// Beam search bookkeeping on the host, free of HIP so that it builds and is tested on a CPU:
// pooling and ordering the candidates of a clip's live beams, assigning them to beam positions, the list of
// self-cache copies a re-parenting needs (with the common-prefix rule) and its schedule for the gather kernel
// (kernels/beam.hip), and the choice of the winner. The per-token rules (timestamps, completion, failure) stay
// with the caller: the engine runs process_step on every re-parented beam, as greedy decoding does.
#pragma once
#include <vector>

namespace wm {

constexpr int kBeamMax = 8;  // upstream's WHISPER_MAX_DECODERS

// One candidate of a row after the logits rules; id < 0 or p <= 0: none (a row may have fewer than K)
struct BeamCand {
    int id, tid;
    float p, plog, pt, ptsum;
};

// Beam position `beam` continues beam `parent` with that row's candidate `rank`; parent < 0: the pool ran out,
// the beam at this position has failed
struct BeamPick {
    int beam, parent, rank;
};

// One copy of the self cache: rows [row0, row1) of K and V of every layer and head, slot src -> slot dst.
// mode / stage_off are the gather schedule (beam_schedule): mode 0 = straight from src to dst in the first
// launch, 1 = through the staging buffer (read in the first launch, written in the second) at stage_off
// (16-byte units).
struct KvCopy {
    int dst_slot, src_slot, row0, row1;
    int mode, pad;
    long stage_off;
};

// Contract points 4 and 5. `rows` are the beams that produced candidates (ascending beam index; the prefill row
// counts as beam 0), sum_all[r] the sum_logprobs_all of rows[r], cands[r * K + j] its candidates in rank order.
// The pool is ordered by (sum_all + plog descending, parent index ascending, rank ascending) and its first
// positions.size() entries go to `positions` in the order given; a position beyond the pool gets parent -1.
std::vector<BeamPick> beam_select(const std::vector<int>& rows, const std::vector<double>& sum_all,
                                  const BeamCand* cands, int K, const std::vector<int>& positions);

// The copies that make every picked position's self slot hold its parent's rows. held[b] = the token sequence
// (prompt included) whose K/V rows slot slots[b] holds; row p depends on tokens 0..p only, so a destination
// that agrees with its source on the first m tokens keeps rows < m and receives rows [m, held[parent].size()).
// Parallel assignment: every copy reads the cache as it was before; held is updated the same way.
std::vector<KvCopy> beam_copies(const std::vector<BeamPick>& picks, std::vector<std::vector<int>>& held,
                                const std::vector<int>& slots);

// Schedule for the gather kernel: a copy whose destination slot no copy of the list reads goes straight
// (mode 0), the others (chains, swaps, cycles) through the staging buffer (mode 1, stage_off assigned).
// units_per_row = 16-byte units of one cache row over all layers, K and V, heads (L * 2 * H * 8).
// Returns the staging buffer's size in 16-byte units.
long beam_schedule(std::vector<KvCopy>& copies, long units_per_row);

// Contract point 6: the highest score among beams that have not failed, lowest index on ties; -1: none
int beam_winner(const std::vector<double>& score, const std::vector<char>& failed);

}  // namespace wm
