/* spans_ref.cpp -- writes what the REFERENCE computes for the fixture of mdbg_kminmer_spans.  Used only to regenerate
 * tests/golden/kminmer_spans (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only #includes the
 * reference's Commons.hpp and calls its EncoderRLE::execute (Commons.hpp:4163-4203), MinimizerParser::parse (utils/kmer/Kmer.hpp:1373-1456)
 * and MDBG::getKminmers (Commons.hpp:5401-5526).
 *
 *   spans_ref <l> <density> <hpc> <trim> <k>  < reads, one per line
 *
 * Output, one line each:
 *   R <read> <minimizers> <windows>
 *   M <read> <value> <pos> <rle[pos]> <rle[pos + l]>
 *   W <read> <reversed> <hash_hi> <hash_lo> <read_pos_start> <read_pos_end> <length> <seq_length_start> <seq_length_end> <the four position fields>
 * Without compression the reference's rlePositions has no entry at the read's length; a minimizer that would need it (no end trim and
 * the last l-mer selected) makes the program stop: the fixture must not contain that case. */
#include "Commons.hpp"

#include <iostream>
#include <string>

int main(int argc, char **argv)
{
    if (argc < 6) { std::cerr << "usage: spans_ref <l> <density> <hpc> <trim> <k>\n"; return 2; }
    const size_t l = std::stoul(argv[1]);
    const float density = std::stof(argv[2]);
    const bool hpc = std::stoi(argv[3]) != 0;
    const size_t trim = std::stoul(argv[4]);
    const size_t k = std::stoul(argv[5]);
    unordered_set<MinimizerType> rep;
    MinimizerParser parser(l, density, rep);
    parser._trimBps = trim;
    EncoderRLE enc;
    std::string line;
    size_t r = 0;
    while (std::getline(std::cin, line)) {
        std::string rle;
        vector<u_int64_t> rlePos;
        enc.execute(line.c_str(), line.size(), rle, rlePos, hpc);
        vector<MinimizerType> m;
        vector<u_int32_t> pos;
        vector<u_int8_t> dir;
        parser.parse(rle, m, pos, dir);
        vector<KmerVec> kminmers;
        vector<ReadKminmer> info;
        for (size_t i = 0; i < m.size(); i++)
            if (pos[i] + l >= rlePos.size()) { std::cerr << "read " << r << ": rlePositions[" << pos[i] + l << "] does not exist\n"; return 1; }
        MDBG::getKminmers(l, k, m, pos, kminmers, info, rlePos, (int)r, false);
        std::cout << "R " << r << " " << m.size() << " " << kminmers.size() << "\n";
        for (size_t i = 0; i < m.size(); i++)
            std::cout << "M " << r << " " << m[i] << " " << pos[i] << " " << rlePos[pos[i]] << " " << rlePos[pos[i] + l] << "\n";
        for (size_t i = 0; i < kminmers.size(); i++) {
            const u_int128_t h = kminmers[i].hash128();
            const ReadKminmer &q = info[i];
            std::cout << "W " << r << " " << (q._isReversed ? 1 : 0) << " " << (uint64_t)(h >> 64) << " " << (uint64_t)h << " " << q._read_pos_start << " "
                      << q._read_pos_end << " " << q._length << " " << q._seq_length_start << " " << q._seq_length_end << " " << q._position_of_second_minimizer
                      << " " << q._position_of_second_to_last_minimizer << " " << q._position_of_second_minimizer_seq << " "
                      << q._position_of_second_to_last_minimizer_seq << "\n";
        }
        r++;
    }
    return 0;
}
