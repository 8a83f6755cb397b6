/* select_ref.cpp -- writes what the REFERENCE selects for the fixture of mdbg_map_select / mdbg_map_select_merge.  Used only to regenerate
 * tests/golden/read_select (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only #includes the
 * reference's readSelection/ReadMapper.hpp and calls its ReadMapper::ReadFunctor, Commons::sortParallel, ReadMapper::createLookupTable,
 * AlignReadsLowDensityFunctor::processAnchors (which chains a group and feeds addAlignmentScore with the reference's own alignmentQueues /
 * alignmentMatches), AlignReadsLowDensityFunctor::chainAnchors (once more per group, to print the candidates) and
 * ReadMapper::mergeAlignmentScore.  The join-and-sort loop (:698-756), the grouping (:779-800) and the drain of the queues (:805-838)
 * live inside AlignReadsLowDensityFunctor::operator(), which goes on to the partition files, and the drain of the merge (:329-355) inside
 * mergeAlignmentPartition, which reads them: their few lines are written out again below, as tests/golden/read_mapper/mapper_ref.cpp does
 * for the join.
 *
 * The codec: p4nd1enc32 / p4nd1dec32 (ext/TurboPFor-Integer-Compression) are NOT the reference's here.  Its lib/bitunpack.c and
 * lib/bitutil.c do not compile with one plain cc line (they want the instruction-set flags of its own makefile), so this file defines
 * the two symbols itself as a raw copy of the words.  The selection does not depend on the codec: it only has to give back the list
 * it was given.
 *
 *   select_ref <band> <coverage> <chunks> <scratch directory>  < reads
 *
 * Input: `<n reads>`, then per read `<n> m0 p0 m1 p1 ...` (minimizer, position).  The chunks are the read ranges
 * [c n / chunks, (c + 1) n / chunks).  Output, one record a line:
 *   G query ref_read score n m0 m1 ...    every candidate of the whole set: a group of 3 anchors or more with a chain; score =
 *                                         _nbMatches - _nbDifferencesQuery (:1241), the list is _queryAnchorPositions
 *   W query n r0 r1 ...                   the selection with the whole set as one chunk, per query with a selected read
 *   K chunk query n r0 r1 ...             the selection of every chunk
 *   M query n r0 r1 ...                   the chunks' selections merged (mergeAlignmentScore in chunk order) */
#include "readSelection/ReadMapper.hpp"

#include <iostream>

extern "C" {
size_t p4nd1enc32(uint32_t *__restrict in, size_t n, unsigned char *__restrict out) { memcpy(out, in, n * 4); return n * 4; }
size_t p4nd1dec32(unsigned char *__restrict in, size_t n, uint32_t *__restrict out) { memcpy(out, in, n * 4); return n * 4; }
}

typedef vector<vector<ReadMapper::AlignmentScoreMatches>> ChunkResult;      /* per query, sorted by read */

static ChunkResult run_chunk(const std::vector<KminmerList> &reads, size_t lo, size_t hi, u_int64_t band, u_int64_t coverage, const std::string &dir, std::ostream *candidates)
{
    ReadMapper mapper(dir, dir + "/alignments.bin", reads.size(), band, coverage, 1ull << 40, 0, 1);
    mapper._kminmerSize = 2;
    mapper._nbReadsProcessed = 0;
    mapper._nbReadsInChunk = 0;
    ReadMapper::ReadFunctor load(mapper);
    for (size_t r = lo; r < hi; r++) load(reads[r]);
    Commons::sortParallel(mapper._allMinimizerPositions, mapper._allMinimizerPositions.size(), 1);
    mapper.createLookupTable();
    ReadMapper::AlignReadsLowDensityFunctor align(mapper);
    ChunkResult result(reads.size());
    for (const KminmerList &kminmerList : reads) {
        MinimizerRead read = {kminmerList._readIndex, kminmerList._readMinimizers, kminmerList._minimizerPos, kminmerList._readQualities, kminmerList._readMinimizerDirections, kminmerList._readLength};
        if (Utils::isReadTooShort(read)) continue;
        vector<ReadMapper::Anchor2> anchors;
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
        /* ---- :772-800: the groups, each through the reference's processAnchors ---- */
        vector<ReadMapper::AlignmentMatches> alignmentMatches;
        vector<ReadMapper::AlignmentScoreQueue> alignmentQueues(read._minimizers.size());
        for (size_t h = 0; h < anchors.size();) {
            size_t t = h;
            while (t < anchors.size() && anchors[t]._readIndex == anchors[h]._readIndex) t++;
            const vector<ReadMapper::Anchor2> subAnchors(anchors.begin() + h, anchors.begin() + t);
            align.processAnchors(subAnchors, read, anchors[h]._readIndex, alignmentQueues, alignmentMatches);
            if (candidates && subAnchors.size() >= 3) {
                ReadMapper::Chain2 chain = align.chainAnchors(subAnchors, read, (int64_t)band, anchors[h]._readIndex);
                if (chain._chainingScore != 0) {
                    *candidates << "G " << read._readIndex << " " << anchors[h]._readIndex << " " << (int32_t)(chain._nbMatches - chain._nbDifferencesQuery) << " "
                                << chain._queryAnchorPositions.size();
                    for (u_int32_t m : chain._queryAnchorPositions) *candidates << " " << m;
                    *candidates << "\n";
                }
            }
            h = t;
        }
        /* ---- :805-838: the drain ---- */
        ankerl::unordered_dense::map<ReadType, ReadMapper::AlignmentScoreMatches> selectedAlignments;
        for (ReadMapper::AlignmentScoreQueue &queue : alignmentQueues) {
            while (queue.size() > 0) {
                const ReadMapper::AlignmentScore &alignmentScore = queue.top();
                selectedAlignments[alignmentScore._queryReadIndex] = {alignmentScore._queryReadIndex, 0, {}};
                queue.pop();
            }
        }
        for (const ReadMapper::AlignmentMatches &matches : alignmentMatches) {
            if (selectedAlignments.find(matches._readIndex) == selectedAlignments.end()) continue;
            selectedAlignments[matches._readIndex]._nbMatches = matches._nbMatches;
            selectedAlignments[matches._readIndex]._compressedMatchPositions = matches._compressedMatchPositions;
        }
        vector<ReadMapper::AlignmentScoreMatches> &selectedAlignmentsVec = result[read._readIndex];
        for (const auto &it : selectedAlignments) selectedAlignmentsVec.push_back(it.second);
        std::sort(selectedAlignmentsVec.begin(), selectedAlignmentsVec.end(), [](const ReadMapper::AlignmentScoreMatches &a, const ReadMapper::AlignmentScoreMatches &b) {
            return a._queryReadIndex < b._queryReadIndex;
        });
    }
    return result;
}

static void print(std::ostream &out, const std::string &tag, const ChunkResult &result)
{
    for (size_t q = 0; q < result.size(); q++) {
        if (result[q].empty()) continue;
        out << tag << " " << q << " " << result[q].size();
        for (const auto &al : result[q]) out << " " << al._queryReadIndex;
        out << "\n";
    }
}

int main(int argc, char **argv)
{
    if (argc < 5) { std::cerr << "usage: select_ref <band> <coverage> <chunks> <scratch directory> < reads\n"; return 2; }
    const u_int64_t band = std::stoull(argv[1]), coverage = std::stoull(argv[2]);
    const size_t n_chunks = std::stoull(argv[3]);
    const std::string dir = argv[4];
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
    std::ostringstream out;
    print(out, "W", run_chunk(reads, 0, n_reads, band, coverage, dir, &out));
    std::vector<ChunkResult> chunks;
    for (size_t c = 0; c < n_chunks; c++) {
        chunks.push_back(run_chunk(reads, c * n_reads / n_chunks, (c + 1) * n_reads / n_chunks, band, coverage, dir, nullptr));
        print(out, "K " + std::to_string(c), chunks.back());
    }
    /* ---- mergeAlignmentPartition :317-358: the chunks' alignments of a read in chunk order through mergeAlignmentScore, then the drain ---- */
    ReadMapper merger(dir, dir + "/alignments.bin", n_reads, band, coverage, 1ull << 40, 0, 1);
    ChunkResult merged(n_reads);
    for (size_t q = 0; q < n_reads; q++) {
        vector<ReadMapper::AlignmentScoreQueue> alignmentQueues;
        for (const ChunkResult &chunk : chunks)
            for (const ReadMapper::AlignmentScoreMatches &alignment : chunk[q]) merger.mergeAlignmentScore((ReadType)q, alignment, alignmentQueues);
        ankerl::unordered_dense::map<ReadType, ReadMapper::AlignmentScore> selectedAlignments;
        for (ReadMapper::AlignmentScoreQueue &queue : alignmentQueues) {
            while (queue.size() > 0) {
                const ReadMapper::AlignmentScore &alignmentScore = queue.top();
                selectedAlignments[alignmentScore._queryReadIndex] = alignmentScore;
                queue.pop();
            }
        }
        for (const auto &it : selectedAlignments) merged[q].push_back({it.second._queryReadIndex, 0, {}});
        std::sort(merged[q].begin(), merged[q].end(), [](const ReadMapper::AlignmentScoreMatches &a, const ReadMapper::AlignmentScoreMatches &b) {
            return a._queryReadIndex < b._queryReadIndex;
        });
    }
    print(out, "M", merged);
    std::cout << out.str();
    return 0;
}
