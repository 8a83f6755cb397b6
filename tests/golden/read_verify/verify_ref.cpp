/* verify_ref.cpp -- writes what the REFERENCE computes for the fixture of mdbg_map_verify.  Used only to regenerate tests/golden/read_verify
 * (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only #includes the reference's
 * readSelection/MinimizerChainer.hpp and calls its MinimizerChainer::computeChainingAlignment on the anchors of every (target, neighbour) row.
 * The anchors are what ReadCorrectionFunctor::filterAlignments (ReadCorrection.hpp:5051-5069) hands to it -- one per pair of equal
 * minimizers, the target in the reference's role, the neighbour in the query's; that loop lives inside a functor bound to the whole of
 * ReadCorrection, so the pairing is written here in our own words -- and the verdict is the four tests of :5088-5094 with the thresholds as
 * arguments.
 *
 *   verify_ref <band> <max_overhang> <min_overlap_length> <min_identity> <minimizer_size>  < input
 *
 * Input: `<n reads>`, per read `<n> <raw length> m0 p0 d0 m1 p1 d1 ...` (minimizer, position, direction), then `<n targets>`, per target
 * `<target read> <k> neighbour0 ... neighbour(k-1)`.  Output, one line a row:
 *   R n_anchors chain query_reversed n_matches n_mismatches n_deletions n_insertions identity_bits overhang_start overhang_end align_length
 *     reference_start reference_end query_start query_end kept
 * (chain: the result carries an alignment; identity_bits: the float _identity as its 32 bits), and at the end `T seconds` for the calls of
 * computeChainingAlignment on one thread. */
#include "readSelection/MinimizerChainer.hpp"

#include <chrono>
#include <cstring>
#include <iostream>
#include <map>

int main(int argc, char **argv)
{
    if (argc < 6) { std::cerr << "usage: verify_ref <band> <max_overhang> <min_overlap_length> <min_identity> <minimizer_size> < input\n"; return 2; }
    const int64_t band = std::stoll(argv[1]);
    const u_int32_t max_overhang = (u_int32_t)std::stoul(argv[2]);
    const float min_overlap = (float)std::stoul(argv[3]);
    const float min_identity = std::stof(argv[4]);
    MinimizerChainer chainer(std::stoul(argv[5]));

    size_t n_reads = 0;
    std::cin >> n_reads;
    std::vector<MinimizerRead> reads(n_reads);
    for (size_t r = 0; r < n_reads; r++) {
        size_t n = 0;
        u_int64_t length = 0;
        std::cin >> n >> length;
        MinimizerRead &read = reads[r];
        read._readIndex = (ReadType)r;
        read._readLength = (u_int32_t)length;
        read._meanReadQuality = 0;
        for (size_t i = 0; i < n; i++) {
            u_int64_t m, p, d;
            std::cin >> m >> p >> d;
            read._minimizers.push_back((MinimizerType)m);
            read._minimizersPos.push_back((u_int32_t)p);
            read._readMinimizerDirections.push_back((u_int8_t)d);
            read._qualities.push_back(0);
        }
    }
    double seconds = 0;
    std::ostringstream out;
    size_t n_targets = 0;
    std::cin >> n_targets;
    for (size_t t = 0; t < n_targets; t++) {
        size_t target = 0, k = 0;
        std::cin >> target >> k;
        const MinimizerRead &tr = reads[target];
        std::map<MinimizerType, std::vector<u_int32_t>> where;              // a target minimizer -> its indexes, ascending
        for (u_int32_t i = 0; i < tr._minimizers.size(); i++) where[tr._minimizers[i]].push_back(i);
        for (size_t s = 0; s < k; s++) {
            size_t neighbour = 0;
            std::cin >> neighbour;
            const MinimizerRead &nr = reads[neighbour];
            std::vector<Anchor> anchors;
            for (u_int32_t j = 0; j < nr._minimizers.size(); j++) {
                const auto hit = where.find(nr._minimizers[j]);
                if (hit == where.end()) continue;
                for (u_int32_t i : hit->second)
                    anchors.push_back(Anchor((int32_t)tr._minimizersPos[i], (int32_t)nr._minimizersPos[j], tr._readMinimizerDirections[i] != nr._readMinimizerDirections[j],
                                             (int32_t)i, (int32_t)j));
            }
            const size_t n_anchors = anchors.size();
            const auto t0 = std::chrono::steady_clock::now();
            AlignmentResult2 a = chainer.computeChainingAlignment(anchors, tr, nr, band);
            seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const bool chain = !a._alignments.empty();
            const bool kept = !(a._overHangStart > max_overhang) && !(a._overHangEnd > max_overhang) && !(a._alignLength < min_overlap) && !(a._identity < min_identity) && chain;
            u_int32_t bits = 0;
            std::memcpy(&bits, &a._identity, 4);
            out << "R " << n_anchors << " " << (int)chain << " " << (chain ? (int)a._isQueryReversed : 0) << " " << a._nbMatches << " " << a._nbMissmatches << " " << a._nbDeletions << " "
                << a._nbInsertions << " " << bits << " " << a._overHangStart << " " << a._overHangEnd << " " << a._alignLength << " " << a._referenceStart << " "
                << a._referenceEnd << " " << a._queryStart << " " << a._queryEnd << " " << (int)kept << "\n";
        }
    }
    out << "T " << seconds << "\n";
    std::cout << out.str();
    return 0;
}
