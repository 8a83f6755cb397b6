/* mapper_ref.cpp -- writes what the REFERENCE computes for the fixture of mdbg_map_index_build / mdbg_map_anchors / mdbg_map_chains.  Used
 * only to regenerate tests/golden/read_mapper (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only
 * #includes the reference's readSelection/ReadMapper.hpp and calls its MDBG::getKminmers_complete (the windows at k = 2),
 * ReadMapper::ReadFunctor (the index entries), Commons::sortParallel, ReadMapper::createLookupTable and
 * ReadMapper::AlignReadsLowDensityFunctor::chainAnchors.  The join-and-sort loop of AlignReadsLowDensityFunctor::operator() (:698-756)
 * lives inside that operator, which goes on to the heaps and the partition files, so its fifteen lines are written out again below.
 *
 *   mapper_ref <band> <scratch directory> [summary]  < reads        (summary: only the T line and an N line of counts -- for timing a large set)
 *
 * Input: `<n reads>`, then per read `<n> m0 p0 m1 p1 ...` (minimizer, position).  Output, one record a line:
 *   I pair read position index reversed                  every entry of the sorted index, in its order
 *   Q read n_anchors                                     per query read (0 for a read Utils::isReadTooShort sends away)
 *   A ref_read ref_position ref_index query_position query_index reversed        its anchors, sorted
 *   P ref_read n_anchors score                           per (query, reference read) group, chainAnchors called on EVERY group, also
 *                                                        those of fewer than 3 anchors that processAnchors (:850) drops; score 0: no chain
 *   C n_matches query_reversed n_diff_query n_diff_reference query_start query_end reference_start reference_end n m0 m1 ...
 *                                                        behind a P with a score: Chain2's fields and _queryAnchorPositions
 *   T seconds                                            time of index + join + sort + chains on one thread, without this program's own text, for scale
 *   N entries anchors groups chains                      (summary only) */
#include "readSelection/ReadMapper.hpp"

#include <chrono>
#include <iostream>

int main(int argc, char **argv)
{
    if (argc < 3) { std::cerr << "usage: mapper_ref <band> <scratch directory> < reads\n"; return 2; }
    const u_int64_t band = std::stoull(argv[1]);
    const std::string dir = argv[2];
    const bool summary = argc > 3;
    double seconds = 0;
    u_int64_t n_anchors = 0, n_groups = 0, n_chains = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); };
    size_t n_reads = 0;
    std::cin >> n_reads;
    std::vector<KminmerList> reads(n_reads);
    for (size_t r = 0; r < n_reads; r++) {
        size_t n = 0;
        std::cin >> n;
        KminmerList &kl = reads[r];
        kl._readIndex = (ReadType)r;
        kl._readMinimizers.resize(n);
        kl._minimizerPos.resize(n);
        for (size_t i = 0; i < n; i++) { u_int64_t m, p; std::cin >> m >> p; kl._readMinimizers[i] = (MinimizerType)m; kl._minimizerPos[i] = (u_int32_t)p; }
        kl._readQualities.assign(n, 0);
        kl._readMinimizerDirections.assign(n, 0);
        kl._readLength = n ? kl._minimizerPos[n - 1] + 1 : 0;
        MDBG::getKminmers_complete(2, kl._readMinimizers, kl._minimizerPos, kl._kminmersInfo, (int)r, kl._readQualities);
    }
    auto t0 = now();
    ReadMapper mapper(dir, dir + "/alignments.bin", n_reads, band, 20, 1ull << 40, 0, 1);
    mapper._kminmerSize = 2;
    mapper._nbReadsProcessed = 0;
    mapper._nbReadsInChunk = 0;
    ReadMapper::ReadFunctor load(mapper);
    for (const KminmerList &kl : reads) load(kl);
    Commons::sortParallel(mapper._allMinimizerPositions, mapper._allMinimizerPositions.size(), 1);
    mapper.createLookupTable();
    seconds += since(t0);
    std::ostringstream out;
    if (!summary) for (const auto &e : mapper._allMinimizerPositions)
        out << "I " << (u_int64_t)e._minimizerPair << " " << e._readIndex << " " << e._position << " " << e._positionIndex << " " << (int)e._isReversed << "\n";

    ReadMapper::AlignReadsLowDensityFunctor align(mapper);
    for (const KminmerList &kminmerList : reads) {
        MinimizerRead read = {kminmerList._readIndex, kminmerList._readMinimizers, kminmerList._minimizerPos, kminmerList._readQualities, kminmerList._readMinimizerDirections, kminmerList._readLength};
        if (Utils::isReadTooShort(read)) { if (!summary) out << "Q " << kminmerList._readIndex << " 0\n"; continue; }
        vector<ReadMapper::Anchor2> anchors;
        t0 = now();
        /* ---- AlignReadsLowDensityFunctor::operator() :698-756 ---- */
        for (u_int32_t i = 0; i < kminmerList._kminmersInfo.size(); i++) {
            const ReadKminmerComplete &kminmerInfo = kminmerList._kminmersInfo[i];
            const MinimizerPairType minimizerPair = kminmerInfo._vec.packPair();
            bool queryIsReversed = kminmerInfo._isReversed;
            u_int32_t queryPosition = (kminmerList._minimizerPos[i] + kminmerList._minimizerPos[i + 1]) / 2;
            if (mapper._minimizerLookupTable.find(minimizerPair) == mapper._minimizerLookupTable.end()) continue;
            const auto &range = mapper._minimizerLookupTable[minimizerPair];
            for (size_t j = range.first; j <= range.second; j++) {
                const ReadMapper::MinimizerPosition2 &mPos = mapper._allMinimizerPositions[j];
                if (kminmerList._readIndex == mPos._readIndex) continue;
                anchors.push_back({mPos._readIndex, mPos._position, mPos._positionIndex, queryPosition, i, mPos._isReversed != queryIsReversed});
            }
        }
        std::sort(anchors.begin(), anchors.end(), [](const ReadMapper::Anchor2 &a, const ReadMapper::Anchor2 &b) {
            if (a._readIndex == b._readIndex) {
                if (a._referencePosition == b._referencePosition) return a._queryPosition < b._queryPosition;
                return a._referencePosition < b._referencePosition;
            }
            return a._readIndex < b._readIndex;
        });
        /* ---- */
        seconds += since(t0);
        n_anchors += anchors.size();
        if (!summary) out << "Q " << kminmerList._readIndex << " " << anchors.size() << "\n";
        if (!summary) for (const auto &a : anchors)
            out << "A " << a._readIndex << " " << a._referencePosition << " " << a._referencePositionIndex << " " << a._queryPosition << " " << a._queryPositionIndex << " "
                << (int)a._isReversed << "\n";
        for (size_t h = 0; h < anchors.size();) {
            size_t t = h;
            while (t < anchors.size() && anchors[t]._readIndex == anchors[h]._readIndex) t++;
            const vector<ReadMapper::Anchor2> sub(anchors.begin() + h, anchors.begin() + t);
            t0 = now();
            ReadMapper::Chain2 chain = align.chainAnchors(sub, read, (int64_t)band, anchors[h]._readIndex);
            seconds += since(t0);
            n_groups++;
            n_chains += chain._chainingScore != 0;
            if (summary) { h = t; continue; }
            out << "P " << anchors[h]._readIndex << " " << sub.size() << " " << (int64_t)chain._chainingScore << "\n";
            if (chain._chainingScore != 0) {
                out << "C " << chain._nbMatches << " " << (int)chain._isQueryReversed << " " << chain._nbDifferencesQuery << " " << chain._nbDifferencesReference << " "
                    << chain._queryStart << " " << chain._queryEnd << " " << chain._referenceStart << " " << chain._referenceEnd << " " << chain._queryAnchorPositions.size();
                for (u_int32_t m : chain._queryAnchorPositions) out << " " << m;
                out << "\n";
            }
            h = t;
        }
    }
    out << "T " << seconds << "\n";
    if (summary) out << "N " << mapper._allMinimizerPositions.size() << " " << n_anchors << " " << n_groups << " " << n_chains << "\n";
    std::cout << out.str();
    return 0;
}
