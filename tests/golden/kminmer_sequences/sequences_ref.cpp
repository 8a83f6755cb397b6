/* sequences_ref.cpp -- writes what the REFERENCE computes for the fixture of mdbg_spans_extract.  Used only to regenerate
 * tests/golden/kminmer_sequences (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only #includes
 * the reference's toBasespace/ToBasespaceGfa.hpp and calls its EncoderRLE::execute (Commons.hpp:4163-4203), MinimizerParser::parse
 * (utils/kmer/Kmer.hpp:1373-1456), MDBG::getKminmers (Commons.hpp:5401-5526), ToBasespaceGfa::extractKminmerSequence
 * (toBasespace/ToBasespaceGfa.hpp:1050-1103) and DnaBitset2 (utils/DnaBitset.hpp:118-242).
 *
 *   sequences_ref <l> <density> <hpc> <trim> <k> <all_upto> <stride>  < reads, one per line
 *
 * Every window of a read of at most <all_upto> bases and every <stride>-th window of a longer read is cut out three times (LoadType
 * Entire, Left, Right).  Output, one line each:
 *   R <read> <minimizers> <windows>
 *   W <read> <reversed> <read_pos_start> <read_pos_end> <seq_length_start> <seq_length_end>                 (every window)
 *   Q <read> <window of the read> <part 0 Entire / 1 Left / 2 Right> <length> <DnaBitset2::_m_data in hex, - when empty> */
#include "toBasespace/ToBasespaceGfa.hpp"

#include <iostream>
#include <string>

int main(int argc, char **argv)
{
    if (argc < 8) { std::cerr << "usage: sequences_ref <l> <density> <hpc> <trim> <k> <all_upto> <stride>\n"; return 2; }
    const size_t l = std::stoul(argv[1]);
    const float density = std::stof(argv[2]);
    const bool hpc = std::stoi(argv[3]) != 0;
    const size_t trim = std::stoul(argv[4]);
    const size_t k = std::stoul(argv[5]);
    const size_t all_upto = std::stoul(argv[6]);
    const size_t stride = std::stoul(argv[7]);
    unordered_set<MinimizerType> rep;
    MinimizerParser parser(l, density, rep);
    parser._trimBps = trim;
    EncoderRLE enc;
    ToBasespaceGfa tool;
    const ToBasespaceGfa::LoadType types[3] = {ToBasespaceGfa::LoadType::Entire, ToBasespaceGfa::LoadType::Left, ToBasespaceGfa::LoadType::Right};
    static const char hex[] = "0123456789abcdef";
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
        for (size_t i = 0; i < info.size(); i++) {
            const ReadKminmer &q = info[i];
            std::cout << "W " << r << " " << (q._isReversed ? 1 : 0) << " " << q._read_pos_start << " " << q._read_pos_end << " " << q._seq_length_start << " "
                      << q._seq_length_end << "\n";
        }
        for (size_t i = 0; i < info.size(); i += (line.size() <= all_upto ? 1 : stride))
            for (int part = 0; part < 3; part++) {
                std::string seq;
                tool.extractKminmerSequence(line.c_str(), info[i], types[part], seq);
                const DnaBitset2 bits(seq);
                std::string h;
                for (uint8_t b : bits._m_data) { h += hex[b >> 4]; h += hex[b & 15]; }
                std::cout << "Q " << r << " " << i << " " << part << " " << seq.size() << " " << (h.empty() ? "-" : h) << "\n";
            }
        r++;
    }
    return 0;
}
