// graph_plan.hpp -- the arithmetic of a `graph` job (mdbg_tool.cpp): where a read set is cut into pieces, which reads a rank takes, which
// bytes of read_data_corrected.txt a range of records is, and which record files a pass writes.  Nothing here touches a file or the
// library, so that a host test (tests/host/test_graph_plan.cpp) can go through it value by value.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace graph_plan {

constexpr size_t MAX_PIECES = 64;      // the exchange among the pieces of one device counts per destination in arrays of 64

enum class Refusal { none, read_above_limit, too_many_pieces };

// The pass in pieces: contiguous read ranges of at most maxMins minimizers each, taken greedily; cuts[p] .. cuts[p + 1] = piece p.
// offs: minimizers before each read, n_reads + 1 entries.  read_above_limit: one read alone exceeds maxMins (cuts is then unfinished);
// too_many_pieces: cuts is complete and says how many.
inline Refusal piece_cuts(const std::vector<uint64_t> &offs, uint64_t maxMins, std::vector<size_t> &cuts) {
    const size_t nReads = offs.size() - 1;
    cuts.assign(1, 0);
    for (size_t r = 0, first = 0; r < nReads; r++) {
        if (offs[r + 1] - offs[r] > maxMins) return Refusal::read_above_limit;
        if (offs[r + 1] - offs[first] > maxMins) { cuts.push_back(r); first = r; }
    }
    cuts.push_back(nReads);
    return cuts.size() - 1 > MAX_PIECES ? Refusal::too_many_pieces : Refusal::none;
}

// the reads [first, second) of rank r of G
inline std::pair<size_t, size_t> rank_range(size_t nReads, int r, int G) { return {nReads * (size_t)r / (size_t)G, nReads * (size_t)(r + 1) / (size_t)G}; }

// Any range of whole "u32 n; u8 circ; u32 m[n]" records is a file of its own: record r starts at byte 5 r + 4 offs[r].
inline std::pair<size_t, size_t> byte_range(const std::vector<uint64_t> &offs, size_t r0, size_t r1) { return {5 * r0 + 4 * (size_t)offs[r0], 5 * r1 + 4 * (size_t)offs[r1]}; }

// The files under `dir` the 20-byte records of a pass go to: the table and its copies (graph/CreateMdbg.cpp:451-464, :515-522).
inline std::vector<std::string> record_files(const std::string &dir, bool firstPass, uint32_t k, size_t firstK) {
    std::vector<std::string> files{dir + "/kminmerData_abundance.txt"};
    if (firstPass) files.push_back(dir + "/kminmerData_abundance_init.txt");
    if (k == firstK + 1) files.push_back(dir + "/kminmerData_abundance_init_k" + std::to_string(firstK + 1) + ".txt");
    return files;
}

}  // namespace graph_plan
