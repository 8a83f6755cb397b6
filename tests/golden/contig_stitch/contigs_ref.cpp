/* contigs_ref.cpp -- writes what the REFERENCE computes for the fixture of mdbg_spans_stitch + mdbg_sequences_to_fasta_bytes.  Used only to
 * regenerate tests/golden/contig_stitch (make_fixture.py drives it); no test runs it.  No reference source is copied: this file only
 * #includes the reference's toBasespace/ToBasespaceGfa.hpp and calls its EncoderRLE::execute, MinimizerParser::parse, MDBG::getKminmers
 * (the windows, exactly as tests/golden/kminmer_sequences/sequences_ref.cpp computes them), ToBasespaceGfa::extractKminmerSequence +
 * DnaBitset2 for the stored pieces, and ToBasespaceGfa::CreateBaseContigsFunctor::operator() (toBasespace/ToBasespaceGfa.hpp:1464-1795).
 *
 *   contigs_ref <l> <density> <hpc> <trim> <k> <contigs file> <output .gz>  < reads, one per line
 *
 * The contigs file: per contig a line `C <name> <circular flag> <n>` and n lines `<read> <window of the read> <contig window reversed>
 * <present>`.  For contig position i the driver fills _contigPosition_to_readPosition[{name, i}] and -- when present -- the map the
 * LoadType names that SetupKminmerSequenceExtractionFunctor (:996-1040) would choose: Entire for position 0, Right for a forward contig
 * window, Left for a reversed one; the stored value is new DnaBitset2(extractKminmerSequence(...)), as ExtractKminmerSequenceFunctor
 * (:1221-1236) stores it.  A piece that is not present is left out of the map.  The maps are emptied between contigs.  The functor
 * writes through _basespaceContigFile, a gzopen()ed file. */
#include "toBasespace/ToBasespaceGfa.hpp"

#include <fstream>
#include <iostream>
#include <string>

int main(int argc, char **argv)
{
    if (argc < 8) { std::cerr << "usage: contigs_ref <l> <density> <hpc> <trim> <k> <contigs file> <output .gz>\n"; return 2; }
    const size_t l = std::stoul(argv[1]);
    const float density = std::stof(argv[2]);
    const bool hpc = std::stoi(argv[3]) != 0;
    const size_t trim = std::stoul(argv[4]);
    const size_t k = std::stoul(argv[5]);
    unordered_set<MinimizerType> rep;
    MinimizerParser parser(l, density, rep);
    parser._trimBps = trim;
    EncoderRLE enc;
    ToBasespaceGfa tool;
    std::vector<std::string> reads;
    std::vector<vector<ReadKminmer>> windows;
    std::string line;
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
        MDBG::getKminmers(l, k, m, pos, kminmers, info, rlePos, (int)reads.size(), false);
        std::cout << "R " << reads.size() << " " << info.size() << "\n";
        reads.push_back(line);
        windows.push_back(info);
    }
    tool._basespaceContigFile = gzopen(argv[7], "wb");
    tool._contigIndex = 0;
    tool._nbBps = 0;
    ToBasespaceGfa::CreateBaseContigsFunctor functor(tool);
    std::ifstream in(argv[6]);
    std::string tag;
    u_int64_t name, circular, n;
    while (in >> tag >> name >> circular >> n) {
        for (auto &kv : tool._readPosition_entire) delete kv.second;
        for (auto &kv : tool._readPosition_left) delete kv.second;
        for (auto &kv : tool._readPosition_right) delete kv.second;
        tool._contigPosition_to_readPosition.clear();
        tool._readPosition_entire.clear();
        tool._readPosition_left.clear();
        tool._readPosition_right.clear();
        KminmerList list;
        list._readIndex = (ReadType)name;
        list._isCircular = (u_int8_t)circular;
        for (u_int32_t i = 0; i < n; i++) {
            u_int32_t read, window, reversed, present;
            in >> read >> window >> reversed >> present;
            if (read >= reads.size() || window >= windows[read].size()) { std::cerr << "contig " << name << ": no window " << window << " of read " << read << "\n"; return 1; }
            ReadKminmerComplete info{};
            info._isReversed = reversed != 0;
            list._kminmersInfo.push_back(info);
            tool._contigPosition_to_readPosition[ContigPosition{(u_int32_t)name, i}] = ToBasespaceGfa::ReadPositionMatch{read, window, 1};
            if (!present) continue;
            const ReadPosition at{read, window};
            const ToBasespaceGfa::LoadType type = i == 0 ? ToBasespaceGfa::LoadType::Entire : reversed ? ToBasespaceGfa::LoadType::Left : ToBasespaceGfa::LoadType::Right;
            std::string seq;
            tool.extractKminmerSequence(reads[read].c_str(), windows[read][window], type, seq);
            (i == 0 ? tool._readPosition_entire : reversed ? tool._readPosition_left : tool._readPosition_right)[at] = new DnaBitset2(seq);
        }
        functor(list);
    }
    gzclose(tool._basespaceContigFile);
    return 0;
}
