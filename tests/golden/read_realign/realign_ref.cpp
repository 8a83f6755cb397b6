/* realign_ref.cpp -- writes what the REFERENCE computes for the fixture of mdbg_map_realign.  Used only to regenerate
 * tests/golden/read_realign (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only #includes the
 * reference's readSelection/MinimizerChainer.hpp and calls its own Utils::getLowDensityMinimizerRead, Utils::isReadTooShort,
 * MinimizerRead::toReverseComplement and MinimizerChainer::computeChainingAlignment (which ends in its normalizeAlignment).  The two loops
 * that pair the reads -- ReadCorrectionFunctor::filterAlignments (ReadCorrection.hpp:5051-5069) at correction density, which decides the
 * kept rows and their flags, and performPoaCorrection4 (:5240-5285) at assembly density -- live inside a functor bound to the whole of
 * ReadCorrection, so the pairing is written here in our own words.
 *
 *   realign_ref <band> <max_overhang> <min_overlap_length> <min_identity> <minimizer_size> <assembly_density> <flip_every>  < input
 *
 * Input: `<n reads>`, per read `<n> <raw length> m0 p0 d0 q0 m1 p1 d1 q1 ...` (minimizer, position, direction, quality), then `<n targets>`,
 * per target `<target read> <k> neighbour0 ... neighbour(k-1)`.  Every flip_every-th kept row (counted over the whole input, the first
 * being row flip_every - 1) has its flag flipped on purpose.  Output:
 *   D <read> <n thinned> i0 i1 ...                 the indexes of the minimizers the reference's thinning keeps
 *   K <target> <neighbour> <flag given> <flipped> <state> <n_anchors> <chain_reversed> <n_matches> <n_mismatches> <n_deletions> <n_insertions>
 *     <reference_start_index> <reference_end_index> <n_entries> <checksum> then per entry <ref_index> <query_index> (-1 none) <kind> <quality>
 *     (state: 0 no chain, 1 chain, 16 the thinned neighbour is too short; kind: 0 equal minimizers, 1 different, 2 no ref_index, 3 no
 *     query_index; quality is what addAlignment2 reads: the ORIENTED neighbour's at query_index, 0 for none; checksum: the sum over the
 *     entries k = 0, 1, ... that have a query_index of (k + 1) * the ORIENTED neighbour's minimizer there, mod 2^32 -- the minimizers
 *     themselves would not fit the fixture's size)
 *   T <seconds>                                    the calls of computeChainingAlignment of the second loop, one thread */
#include "readSelection/MinimizerChainer.hpp"

#include <chrono>
#include <iostream>
#include <map>

static std::vector<Anchor> pair_anchors(const MinimizerRead &tr, const MinimizerRead &nr)
{
    std::map<MinimizerType, std::vector<u_int32_t>> where;              // a target minimizer -> its indexes, ascending
    for (u_int32_t i = 0; i < tr._minimizers.size(); i++) where[tr._minimizers[i]].push_back(i);
    std::vector<Anchor> anchors;
    for (u_int32_t j = 0; j < nr._minimizers.size(); j++) {
        const auto hit = where.find(nr._minimizers[j]);
        if (hit == where.end()) continue;
        for (u_int32_t i : hit->second)
            anchors.push_back(Anchor((int32_t)tr._minimizersPos[i], (int32_t)nr._minimizersPos[j], tr._readMinimizerDirections[i] != nr._readMinimizerDirections[j], (int32_t)i,
                                     (int32_t)j));
    }
    return anchors;
}

int main(int argc, char **argv)
{
    if (argc < 8) { std::cerr << "usage: realign_ref <band> <max_overhang> <min_overlap_length> <min_identity> <minimizer_size> <assembly_density> <flip_every> < input\n"; return 2; }
    const int64_t band = std::stoll(argv[1]);
    const u_int32_t max_overhang = (u_int32_t)std::stoul(argv[2]);
    const float min_overlap = (float)std::stoul(argv[3]);
    const float min_identity = std::stof(argv[4]);
    MinimizerChainer chainer(std::stoul(argv[5]));
    const float density = std::stof(argv[6]);
    const size_t flip_every = std::stoul(argv[7]);

    size_t n_reads = 0;
    std::cin >> n_reads;
    std::vector<MinimizerRead> reads(n_reads), thinned(n_reads);
    std::ostringstream out;
    for (size_t r = 0; r < n_reads; r++) {
        size_t n = 0;
        u_int64_t length = 0;
        std::cin >> n >> length;
        MinimizerRead &read = reads[r];
        read._readIndex = (ReadType)r;
        read._readLength = (u_int32_t)length;
        read._meanReadQuality = 0;
        for (size_t i = 0; i < n; i++) {
            u_int64_t m, p, d, q;
            std::cin >> m >> p >> d >> q;
            read._minimizers.push_back((MinimizerType)m);
            read._minimizersPos.push_back((u_int32_t)p);
            read._readMinimizerDirections.push_back((u_int8_t)d);
            read._qualities.push_back((u_int8_t)q);
        }
        thinned[r] = Utils::getLowDensityMinimizerRead(read, density);
        out << "D " << r << " " << thinned[r]._minimizers.size();
        for (size_t i = 0, k = 0; i < n && k < thinned[r]._minimizers.size(); i++)          // positions rise strictly: they name the kept minimizers
            if (read._minimizersPos[i] == thinned[r]._minimizersPos[k]) { out << " " << i; k++; }
        out << "\n";
    }
    double seconds = 0;
    size_t n_targets = 0, n_kept = 0;
    std::cin >> n_targets;
    for (size_t t = 0; t < n_targets; t++) {
        size_t target = 0, k = 0;
        std::cin >> target >> k;
        const MinimizerRead &tr = reads[target];
        const MinimizerRead &tt = thinned[target];
        for (size_t s = 0; s < k; s++) {
            size_t neighbour = 0;
            std::cin >> neighbour;
            // the verify step at correction density: kept or not, and the flag
            std::vector<Anchor> anchors = pair_anchors(tr, reads[neighbour]);
            AlignmentResult2 a = chainer.computeChainingAlignment(anchors, tr, reads[neighbour], band);
            if (a._alignments.empty()) continue;
            if (a._overHangStart > max_overhang || a._overHangEnd > max_overhang || a._alignLength < min_overlap || a._identity < min_identity) continue;
            bool flag = a._isQueryReversed;
            const bool flipped = flip_every && (n_kept + 1) % flip_every == 0;
            n_kept++;
            if (flipped) flag = !flag;
            // the realign step at assembly density
            MinimizerRead nn = thinned[neighbour];
            out << "K " << target << " " << neighbour << " " << (int)flag << " " << (int)flipped;
            if (Utils::isReadTooShort(nn)) { out << " 16 0 0 0 0 0 0 0 0 0 0\n"; continue; }
            if (flag) nn = nn.toReverseComplement();
            std::vector<Anchor> low = pair_anchors(tt, nn);
            const size_t n_anchors = low.size();
            const auto t0 = std::chrono::steady_clock::now();
            AlignmentResult2 b = chainer.computeChainingAlignment(low, tt, nn, band);
            seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const bool chain = !b._alignments.empty();
            if (!chain) { out << " 0 " << n_anchors << " 0 0 0 0 0 0 0 0 0\n"; continue; }
            u_int32_t checksum = 0;
            for (size_t k = 0; k < b._alignments.size(); k++)
                if (b._alignments[k].second != (u_int32_t)-1) checksum += (u_int32_t)(k + 1) * (u_int32_t)nn._minimizers[b._alignments[k].second];
            out << " 1 " << n_anchors << " " << (int)b._isQueryReversed << " " << b._nbMatches << " " << b._nbMissmatches << " " << b._nbDeletions << " " << b._nbInsertions << " "
                << b._referenceStartIndex << " " << b._referenceEndIndex << " " << b._alignments.size() << " " << checksum;
            for (const auto &e : b._alignments) {
                const bool has_r = e.first != (u_int32_t)-1, has_q = e.second != (u_int32_t)-1;
                const int kind = !has_r ? 2 : !has_q ? 3 : tt._minimizers[e.first] == nn._minimizers[e.second] ? 0 : 1;
                out << " " << (int64_t)(int32_t)e.first << " " << (int64_t)(int32_t)e.second << " " << kind << " " << (has_q ? (int)nn._qualities[e.second] : 0);
            }
            out << "\n";
        }
    }
    out << "T " << seconds << "\n";
    std::cout << out.str();
    return 0;
}
