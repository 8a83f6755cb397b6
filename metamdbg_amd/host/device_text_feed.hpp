// device_text_feed.hpp -- MDBG_TOOL_DEVICE_PARSE=1: plain FASTA / FASTQ files travel as text and are taken apart on the device
// (mdbg_reads_from_fastx_bytes); BGZF files travel compressed and are inflated there first (mdbg_bytes_inflate_bgzf), ordinary gzip
// files too (mdbg_bytes_inflate_gzip).  DeviceParsePlan: what the files of the input list are and whether the device can take them;
// DeviceTextFeed: the slabs of their text, handed to the consumers in read order.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bgzf_slabs.hpp"
#include "hostfeed.hpp"
#include "tool_base.hpp"

// The symbols are looked up weakly: a library without them (the CPU tests' double) means the host feed.
extern "C" int mdbg_reads_from_fastx_bytes(mdbg_ctx *ctx, const mdbg_bytes *text, uint64_t begin, uint64_t end, mdbg_reads **out, uint64_t info[4])
    __attribute__((weak));
extern "C" int mdbg_bytes_inflate_bgzf(mdbg_ctx *ctx, const mdbg_bytes *comp, const mdbg_bgzf_block *blocks, uint64_t n_blocks, mdbg_bytes *text, uint64_t text_at,
                                       uint64_t *n_text) __attribute__((weak));
extern "C" int mdbg_bytes_download(mdbg_ctx *ctx, const mdbg_bytes *b, uint64_t at, void *host, uint64_t n) __attribute__((weak));
extern "C" int mdbg_fastx_whole_records(mdbg_ctx *ctx, const mdbg_bytes *text, uint64_t begin, uint64_t end, uint64_t *cut, int *format) __attribute__((weak));
// gzip that is not BGZF: cut into chunks at deflate block headers found here (mdbg_host::gzip_find_block) and inflated on the device
extern "C" int mdbg_gzip_stream_create(mdbg_ctx *ctx, mdbg_gzip_stream **out) __attribute__((weak));
extern "C" void mdbg_gzip_stream_free(mdbg_gzip_stream *s) __attribute__((weak));
extern "C" int mdbg_bytes_inflate_gzip(mdbg_ctx *ctx, mdbg_gzip_stream *s, const mdbg_bytes *comp, const mdbg_gzip_chunk *chunks, uint64_t n_chunks, mdbg_bytes *text,
                                       uint64_t text_at, uint64_t *n_text, uint64_t info[4]) __attribute__((weak));
extern "C" int mdbg_bytes_copy(mdbg_ctx *ctx, mdbg_bytes *dst, uint64_t dst_at, const mdbg_bytes *src, uint64_t src_at, uint64_t n) __attribute__((weak));

struct DeviceParsePlan {
    // a BGZF file: its mapping, its block table (BgzfReader::index) and the text offset of every block
    struct Bgzf {
        std::string path;
        const unsigned char *addr = nullptr;
        std::vector<mdbg_host::BgzfReader::Block> blocks;
        std::vector<uint64_t> cum;
    };
    // A gzip file that is not BGZF: worker threads look for one deflate block header per `chunk` bytes of the file (start[k]: the first
    // header in chunk k, NONE: none found; start[0] is the file's first member header) and run ahead of the consumers, which inflate
    // groups of chunks on the device (mdbg_bytes_inflate_gzip) and carry the unfinished record from slab to slab.
    struct Gzip {
        static constexpr uint64_t NONE = mdbg_host::GZIP_NONE;
        std::string path;
        const unsigned char *addr = nullptr;
        size_t size = 0, chunk = 65536, nChunks = 0;
        std::vector<uint64_t> start;
        std::vector<char> known;
        std::mutex mu;
        std::condition_variable cv;
        std::atomic<size_t> nextSearch{0};
        std::vector<std::thread> workers;
        // where the consumers stand (under the feed's lock)
        mdbg_gzip_stream *stream = nullptr;
        uint64_t atBit = 0;             // the next call's first start
        size_t nextK = 1;               // the first chunk whose header may lie behind atBit
        mdbg_bytes *rest = nullptr;     // the unfinished record behind the last slab's cut
        uint64_t nRest = 0;
        bool ended = false;
        uint64_t nCalls = 0, nChunksInflated = 0;

        struct Probe { mdbg_host::InflaterT<uint16_t> inflater; std::vector<uint16_t> scratch; };      // what a search works with, from chunk to chunk
        void search(size_t k, Probe &p) {
            const uint64_t found = mdbg_host::gzip_find_block(addr, addr + size, (uint64_t)k * chunk * 8, (uint64_t)(k + 1) * chunk * 8, p.inflater, p.scratch);
            std::lock_guard<std::mutex> g(mu);
            start[k] = found;
            known[k] = 1;
            cv.notify_all();
        }
        void run_workers(int threads) {
            for (int t = 0; t < threads; t++)
                workers.emplace_back([this] {
                    Probe p;
                    for (;;) {
                        const size_t k = nextSearch.fetch_add(1);
                        if (k >= nChunks) return;
                        search(k, p);
                    }
                });
        }
        uint64_t wait_start(size_t k) {
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return known[k] != 0; });
            return start[k];
        }
        void join() { for (auto &t : workers) t.join(); workers.clear(); }
    };
    struct Slab { const char *p; size_t n; int file; int bgzf; int gz; };        // bgzf >= 0: the whole of bgzfs[bgzf], gz >= 0: of gzips[gz], cut into slabs as it is inflated
    std::vector<Slab> slabs;            // whole records each, in read order
    std::vector<Bgzf> bgzfs;
    std::vector<std::unique_ptr<Gzip>> gzips;
    size_t maxSlab = 0;
    std::vector<std::pair<void *, size_t>> maps;

    // The first blocks of a BGZF file inflated on the host, until 256 records or 1 MB of text: what the plain files' checks look at.
    // false: a block of the prefix does not inflate
    static bool bgzf_prefix(const Bgzf &z, std::string &text) {
        mdbg_host::Inflater inf;
        std::vector<uint8_t> buf(65536 + 512);            // the decoder wants Inflater::MIN_ROOM bytes of room in front of every symbol
        size_t lines = 0, headers = 0;
        for (size_t b = 0; b < z.blocks.size() && text.size() < ((size_t)1 << 20) && headers <= 256 && lines < 4 * 256 + 4; b++) {
            const auto &blk = z.blocks[b];
            inf.reset(z.addr + blk.payload, z.addr + blk.payload + blk.csize);
            size_t produced = 0;
            if (inf.run(buf.data(), buf.data() + buf.size(), 0, &produced) != mdbg_host::Inflater::STREAM_END || produced != blk.isize) return false;
            for (size_t i = 0; i < produced; i++) {
                if (buf[i] == '\n') lines++;
                if (buf[i] == '>' && (i ? buf[i - 1] == '\n' : text.empty() || text.back() == '\n')) headers++;
            }
            text.append((const char *)buf.data(), produced);
        }
        return true;
    }

    // The first member of a gzip file inflated on the host, until 1 MB of text: what the plain files' checks look at.  false: it does not inflate
    static bool gzip_prefix(const unsigned char *addr, size_t size, std::string &text) {
        const size_t h = mdbg_host::gzip_header_size(addr, size);
        if (!h) return false;
        mdbg_host::Inflater inf;
        std::vector<uint8_t> buf(((size_t)1 << 20) + 512);
        inf.reset(addr + h, addr + size);
        size_t produced = 0;
        if (inf.run(buf.data(), buf.data() + buf.size(), 0, &produced) == mdbg_host::Inflater::CORRUPT) return false;
        text.assign((const char *)buf.data(), produced);
        return true;
    }
    // a gzip file that is not BGZF joins the plan; false: `why` says what stands against it
    bool add_gzip(const std::string &path, const unsigned char *addr, size_t size, int file, int threads, int gpus, std::string &why) {
        if (!mdbg_bytes_inflate_gzip || !mdbg_gzip_stream_create || !mdbg_gzip_stream_free || !mdbg_bytes_copy) { why = path + " is gzip but not BGZF and the library has no mdbg_bytes_inflate_gzip"; return false; }
        if (gpus > 1) { why = path + " is gzip but not BGZF: its chunks are inflated on one device, and --gpus is " + std::to_string(gpus); return false; }
        std::string head;
        if (!gzip_prefix(addr, size, head)) { why = path + " is gzip but not BGZF and its first member does not inflate"; return false; }
        if (head.empty()) { why = path + " is gzip but not BGZF and begins with an empty member"; return false; }
        const bool fastq = head[0] == '@';
        if (!fastq && head[0] != '>') { why = path + " does not begin with '>' or '@'"; return false; }
        if (fastq && !mdbg_host::ReadFeeder::fastq_is_four_line(head.data(), head.data() + head.size())) { why = path + " is not four-line FASTQ, which the device parse refuses"; return false; }
        std::unique_ptr<Gzip> g(new Gzip());
        g->path = path; g->addr = addr; g->size = size;
        if (const char *e = getenv("MDBG_TOOL_GZIP_CHUNK_KB")) g->chunk = (size_t)std::max(16, atoi(e)) << 10;
        g->nChunks = (size + g->chunk - 1) / g->chunk;
        g->start.assign(g->nChunks, Gzip::NONE);
        g->known.assign(g->nChunks, 0);
        g->start[0] = 0; g->known[0] = 1;
        // a stream of stored blocks has no header the search finds, and would decode on one wave: the host feed takes it
        if (g->nChunks > 2) {
            Gzip::Probe p;
            g->search(1, p); g->search(2, p);
            if (g->start[1] == Gzip::NONE && g->start[2] == Gzip::NONE) {
                why = path + " is gzip but not BGZF, and no deflate block header is to be found in its second and third chunk (stored blocks, or members of one block): it would inflate on one wave of the device";
                return false;
            }
        }
        // A call of few chunks occupies a fraction of the device's waves and still pays a whole chunk's latency on one lane (DESIGN.md
        // 4.3c, 6): a file of fewer than 32 chunks is left to the host feed, which has it decoded before the first call would return.
        if (g->nChunks < 32) {
            why = path + " is gzip but not BGZF and holds " + std::to_string(g->nChunks) + " chunk(s) of " + std::to_string(g->chunk >> 10) +
                  " KB: fewer than the 32 from which the device takes a gzip file";
            return false;
        }
        g->nextSearch = g->nChunks > 2 ? 3 : 1;
        g->run_workers(std::max(1, std::min(threads, 16)));
        slabs.push_back(Slab{nullptr, 0, file, -1, (int)gzips.size()});
        gzips.push_back(std::move(g));
        return true;
    }

    // true: every file of the list is plain text, pure BGZF or ordinary gzip that begins with '>' or '@' (FASTQ: four lines a record).  Plain files are
    // mapped and cut at record starts by the feeder's own search into slabs of at most batchBases bytes; a BGZF file is one entry that
    // the consumers cut as its text appears on the device.  false: `why` says what stands against it
    bool make(const std::vector<std::string> &files, size_t batchBases, int threads, int gpus, std::string &why) {
        using mdbg_host::ReadFeeder;
        if (!mdbg_reads_from_fastx_bytes) { why = "the library has no mdbg_reads_from_fastx_bytes"; return false; }
        for (size_t f = 0; f < files.size(); f++) {
            const std::string &path = files[f];
            const bool gz = ReadFeeder::file_is_gzip(path);
            if (gz && (!mdbg_bytes_inflate_bgzf || !mdbg_bytes_download || !mdbg_fastx_whole_records)) {
                why = path + " is compressed and the library has no mdbg_bytes_inflate_bgzf, mdbg_bytes_download or mdbg_fastx_whole_records";
                return false;
            }
            const int fd = open(path.c_str(), O_RDONLY);
            if (fd < 0) die("File not found: " + path);
            struct stat st;
            fstat(fd, &st);
            if (st.st_size == 0) { close(fd); continue; }
            const char *addr = (const char *)mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            close(fd);
            if (addr == MAP_FAILED) die("mmap failed: " + path);
            madvise((void *)addr, (size_t)st.st_size, MADV_SEQUENTIAL);
            maps.emplace_back((void *)addr, (size_t)st.st_size);
            if (gz) {
                Bgzf z;
                z.path = path;
                z.addr = (const unsigned char *)addr;
                if (!mdbg_host::BgzfReader::index(z.addr, (size_t)st.st_size, z.blocks)) {
                    if (!add_gzip(path, z.addr, (size_t)st.st_size, (int)f, threads, gpus, why)) return false;
                    continue;
                }
                z.cum.assign(z.blocks.size() + 1, 0);
                for (size_t i = 0; i < z.blocks.size(); i++) z.cum[i + 1] = z.cum[i] + z.blocks[i].isize;
                if (z.cum.back() == 0) continue;                        // nothing but empty blocks: no reads
                std::string head;
                if (!bgzf_prefix(z, head)) { why = path + " has a BGZF block among its first that does not inflate"; return false; }
                const bool fastq = head[0] == '@';
                if (!fastq && head[0] != '>') { why = path + " does not begin with '>' or '@'"; return false; }
                if (fastq && !ReadFeeder::fastq_is_four_line(head.data(), head.data() + head.size())) {
                    why = path + " is not four-line FASTQ, which the device parse refuses";
                    return false;
                }
                slabs.push_back(Slab{nullptr, 0, (int)f, (int)bgzfs.size(), -1});
                bgzfs.push_back(std::move(z));
                continue;
            }
            const char *end = addr + st.st_size;
            const bool fastq = *addr == '@';
            if (!fastq && *addr != '>') { why = path + " does not begin with '>' or '@'"; return false; }
            if (fastq && !ReadFeeder::fastq_is_four_line(addr, end)) { why = path + " is not four-line FASTQ, which the device parse refuses"; return false; }
            for (const char *p = addr; p < end;) {
                const char *q = end;
                if ((size_t)(end - p) > batchBases) {
                    q = ReadFeeder::cut_at_record_start(p, p + batchBases, end, fastq);
                    if (q == p) die("a single read is larger than the batch size; raise --batch-bases");
                }
                slabs.push_back(Slab{p, (size_t)(q - p), (int)f, -1, -1});
                maxSlab = std::max(maxSlab, (size_t)(q - p));
                p = q;
            }
        }
        return true;
    }
    void unmap() {
        for (auto &g : gzips) {
            g->nextSearch = g->nChunks;                 // (a plan given up: the searches end with the chunk they are in)
            g->join();
            if (g->rest) mdbg_bytes_free(g->rest);
            if (g->stream) mdbg_gzip_stream_free(g->stream);
            g->rest = nullptr; g->stream = nullptr;
        }
        for (auto &m : maps) munmap(m.first, m.second);
        maps.clear();
    }
    // what the trace says of a plan that stands
    std::string describe() const {
        const std::string head = "device parse: the text of every input file is taken apart on the device, ";
        if (!gzips.empty())
            return head + std::to_string(slabs.size() - bgzfs.size() - gzips.size()) + " slab(s) of plain text, " + std::to_string(bgzfs.size()) + " BGZF file(s) and " +
                   std::to_string(gzips.size()) + " gzip file(s) cut into chunks at deflate block headers, inflated there and cut into slabs";
        if (bgzfs.empty()) return head + std::to_string(slabs.size()) + " slab(s)";
        return head + std::to_string(slabs.size() - bgzfs.size()) + " slab(s) of plain text and " + std::to_string(bgzfs.size()) + " BGZF file(s) cut into slabs as they are inflated there";
    }
};

// The input's text, slab by slab, to whichever consumer asks next: everything below `mu` is read and written under it, so slabs (and,
// without device parse, the host feeder's batches: the consumers take `mu` and `nextSeq` for those too) leave in read order.
struct DeviceTextFeed {
    DeviceParsePlan plan;
    size_t batchText = 1;               // a slab's text at the most (--batch-bases)
    std::mutex mu;
    uint64_t nextSeq = 0;               // the number of the next slab (batch) handed out
    size_t nextSlab = 0;                // in plan.slabs
    mdbg_host::BgzfCursor bgzf;         // where the BGZF file at plan.slabs[nextSlab] stands
    uint64_t bgzfSlabs = 0, bgzfInflated = 0, bgzfBlocks = 0;
    mdbg_ctx *gzCtx = nullptr;          // gzip files are inflated by a context of their own: a stream belongs to one context, the consumers take turns
    uint64_t gzSlabs = 0, gzChunks = 0, gzCalls = 0;

    // a slab on its way to the parser: plan.slabs[idx], as it lies in the mapping (text == null) or [begin, end) of `text` on the device
    struct Handed { uint64_t seq = 0; size_t idx = 0; mdbg_bytes *text = nullptr; uint64_t begin = 0, end = 0; };

    // The next slab in read order; false: the input is at its end.  `ctx`: the asking consumer's context (BGZF is inflated on it);
    // *inflating grows by the time spent inflating.
    bool next(mdbg_ctx *ctx, Handed &h, double *inflating) {
        std::lock_guard<std::mutex> g(mu);
        for (;;) {
            h.idx = nextSlab;
            if (h.idx >= plan.slabs.size()) return false;
            const int zi = plan.slabs[h.idx].bgzf, gi = plan.slabs[h.idx].gz;
            if (gi >= 0) {
                const double t0 = g_trace.now();
                const bool got = next_gzip_slab(*plan.gzips[(size_t)gi], &h.text, &h.begin, &h.end);
                *inflating += g_trace.now() - t0;
                if (got) { gzSlabs++; break; }
                nextSlab++;                          // this file is done
                continue;
            }
            if (zi < 0) { nextSlab++; break; }
            const double t0 = g_trace.now();
            const bool got = next_bgzf_slab(ctx, plan.bgzfs[(size_t)zi], &h.text, &h.begin, &h.end);
            *inflating += g_trace.now() - t0;
            if (got) { bgzfSlabs++; break; }
            bgzfBlocks += plan.bgzfs[(size_t)zi].blocks.size();
            nextSlab++;                              // this file is done
            bgzf = mdbg_host::BgzfCursor{};
        }
        h.seq = nextSeq++;
        return true;
    }

    // The next slab of the BGZF file `z` (mu held: where a slab ends is known only when its text is on the device, and the next
    // begins there).  A slab is a run of blocks of at most batchText bytes of text, and one block more when it begins inside its first
    // block (bgzf_slabs.hpp); its compressed bytes go up from the mapping and are inflated to offset 0 of *text.  All but the file's last
    // slab end behind their last whole record (mdbg_fastx_whole_records); the next slab begins with the block that holds that place,
    // inflated a second time.  Returns false when the file has no text left; otherwise [*begin, *end) of *text is to be parsed.
    // A block that does not inflate ends the run with the library's message: the reads in front of it are already on their way.
    bool next_bgzf_slab(mdbg_ctx *ctx, const DeviceParsePlan::Bgzf &z, mdbg_bytes **text, uint64_t *begin, uint64_t *end) {
        std::vector<mdbg_bgzf_block> table;
        auto inflate = [&](size_t b0, size_t b1) -> uint64_t {
            if (*text) { mdbg_bytes_free(*text); *text = nullptr; }
            const uint64_t base = z.blocks[b0].payload, top = z.blocks[b1 - 1].payload + z.blocks[b1 - 1].csize;
            table.resize(b1 - b0);
            for (size_t i = b0; i < b1; i++) table[i - b0] = mdbg_bgzf_block{z.blocks[i].payload - base, z.blocks[i].csize, z.blocks[i].isize, z.blocks[i].crc, 0};
            mdbg_bytes *comp = nullptr;
            check_on(ctx, mdbg_bytes_create(ctx, top - base, &comp), "mdbg_bytes_create");
            check_on(ctx, mdbg_bytes_create(ctx, std::max<uint64_t>(1, z.cum[b1] - z.cum[b0]), text), "mdbg_bytes_create");
            check_on(ctx, mdbg_bytes_upload_async(ctx, comp, 0, z.addr + base, top - base, nullptr), "mdbg_bytes_upload_async");
            uint64_t n_text = 0;
            const int rc = mdbg_bytes_inflate_bgzf(ctx, comp, table.data(), table.size(), *text, 0, &n_text);
            mdbg_bytes_free(comp);
            if (rc != MDBG_OK)
                die(z.path + ": " + mdbg_last_error(ctx) + " (the table of this call begins with block " + std::to_string(b0) + " of the file, MDBG_TOOL_DEVICE_PARSE)");
            bgzfInflated += b1 - b0;
            return n_text;
        };
        auto whole_records = [&](uint64_t from, uint64_t n_text) -> uint64_t {
            uint64_t cut = from;
            int format = 0;
            check_on(ctx, mdbg_fastx_whole_records(ctx, *text, from, n_text, &cut, &format), "mdbg_fastx_whole_records");
            return cut;
        };
        *text = nullptr;
        const mdbg_host::BgzfNext got = mdbg_host::bgzf_next_slab(z.cum, bgzf, batchText, inflate, whole_records, begin, end);
        if (got == mdbg_host::BgzfNext::SLAB) return true;
        if (*text) { mdbg_bytes_free(*text); *text = nullptr; }
        if (got == mdbg_host::BgzfNext::READ_TOO_LONG) die("a single read is larger than the batch size; raise --batch-bases");
        return false;
    }

    // The next slab of the gzip file `G` (mu held).  A group of chunks -- about a quarter of batchText in compressed bytes, one
    // chunk at the least -- goes up from the mapping and is inflated behind the unfinished record the last slab left
    // (mdbg_bytes_copy); all but the file's last slab end behind their last whole record (mdbg_fastx_whole_records).  The text
    // buffer is sized by a guess; MDBG_ERANGE names the room needed and leaves the stream where it was.  A start the search
    // guessed wrong ends the run with the device's message: nothing is guessed silently.
    bool next_gzip_slab(DeviceParsePlan::Gzip &G, mdbg_bytes **text, uint64_t *begin, uint64_t *end) {
        using Gz = DeviceParsePlan::Gzip;
        auto gz_die = [&](const std::string &what) {
            die(G.path + ": " + what + " -- set MDBG_TOOL_PARSE_ON_HOST=1 (or run without MDBG_TOOL_DEVICE_PARSE) for the host feed");
        };
        if (!gzCtx) {
            if (mdbg_create(0, &gzCtx) != MDBG_OK) die(std::string("mdbg_create (gzip inflation): ") + mdbg_last_error(nullptr));
            g_more_ctx.push_back(gzCtx);
        }
        if (!G.stream) check_on(gzCtx, mdbg_gzip_stream_create(gzCtx, &G.stream), "mdbg_gzip_stream_create");
        for (;;) {
            if (G.ended) {
                if (G.rest) { mdbg_bytes_free(G.rest); G.rest = nullptr; }
                if (G.nRest) gz_die("the file ends inside a record");      // (the last slab is parsed whole: nothing is left behind it)
                return false;
            }
            const uint64_t target = std::max<uint64_t>(G.chunk, batchText / 4);
            std::vector<mdbg_gzip_chunk> table;
            uint64_t cur = G.atBit;
            size_t k = G.nextK;
            for (;;) {
                uint64_t s = Gz::NONE;
                while (k < G.nChunks && s == Gz::NONE) {
                    const uint64_t f = G.wait_start(k++);
                    if (f != Gz::NONE && f > cur) s = f;
                }
                if (s == Gz::NONE) { table.push_back(mdbg_gzip_chunk{cur, MDBG_GZIP_TO_END}); break; }
                table.push_back(mdbg_gzip_chunk{cur, s});
                cur = s;
                if ((s >> 3) - (G.atBit >> 3) >= target) break;
            }
            const uint64_t stop = table.back().stop_bit;
            const uint64_t base = G.atBit >> 3, top = stop == MDBG_GZIP_TO_END ? G.size : (stop + 7) / 8;
            for (mdbg_gzip_chunk &c : table) {
                if (((c.stop_bit == MDBG_GZIP_TO_END ? G.size : (c.stop_bit + 7) / 8) - (c.start_bit >> 3)) > ((uint64_t)1 << 21))
                    gz_die("no deflate block header was found in 2 MB behind bit " + std::to_string(c.start_bit));
                c.start_bit -= base * 8;
                if (c.stop_bit != MDBG_GZIP_TO_END) c.stop_bit -= base * 8;
            }
            mdbg_bytes *comp = nullptr;
            check_on(gzCtx, mdbg_bytes_create(gzCtx, top - base, &comp), "mdbg_bytes_create");
            check_on(gzCtx, mdbg_bytes_upload_async(gzCtx, comp, 0, G.addr + base, top - base, nullptr), "mdbg_bytes_upload_async");
            uint64_t room = G.nRest + 5 * (top - base) + 65536, n_text = 0, info[4] = {0, 0, 0, 0};
            for (int attempt = 0;; attempt++) {
                check_on(gzCtx, mdbg_bytes_create(gzCtx, room, text), "mdbg_bytes_create");
                if (G.nRest) check_on(gzCtx, mdbg_bytes_copy(gzCtx, *text, 0, G.rest, 0, G.nRest), "mdbg_bytes_copy");
                const int rc = mdbg_bytes_inflate_gzip(gzCtx, G.stream, comp, table.data(), table.size(), *text, G.nRest, &n_text, info);
                if (rc == MDBG_OK) break;
                mdbg_bytes_free(*text);
                *text = nullptr;
                if (rc != MDBG_ERANGE || attempt) {
                    mdbg_bytes_free(comp);
                    gz_die(std::string(mdbg_last_error(gzCtx)) + " (the chunks of this call begin at bit " + std::to_string(G.atBit) + " of the file; a chunk start is a guess of the header search)");
                }
                room = G.nRest + n_text;
            }
            mdbg_bytes_free(comp);
            G.nCalls++; G.nChunksInflated += table.size();
            gzCalls++; gzChunks += table.size();
            const uint64_t n = G.nRest + n_text;
            if (G.rest) { mdbg_bytes_free(G.rest); G.rest = nullptr; }
            G.nRest = 0;
            G.atBit = base * 8 + info[3];
            G.nextK = k;
            *begin = 0;
            *end = n;
            if (info[2]) {                                               // the file's last slab is parsed whole
                G.ended = true;
                if (n == 0) { mdbg_bytes_free(*text); *text = nullptr; return false; }
                return true;
            }
            if (stop == MDBG_GZIP_TO_END) gz_die("the device stopped in front of the file's end");
            uint64_t cut = 0;
            int format = 0;
            if (n) check_on(gzCtx, mdbg_fastx_whole_records(gzCtx, *text, 0, n, &cut, &format), "mdbg_fastx_whole_records");
            if (cut < n) {                                               // the unfinished record goes in front of the next text
                check_on(gzCtx, mdbg_bytes_create(gzCtx, n - cut, &G.rest), "mdbg_bytes_create");
                check_on(gzCtx, mdbg_bytes_copy(gzCtx, G.rest, 0, *text, cut, n - cut), "mdbg_bytes_copy");
                G.nRest = n - cut;
            }
            if (cut > 0) { *end = cut; return true; }
            // not one whole record yet: more chunks
            mdbg_bytes_free(*text);
            *text = nullptr;
            if (n > batchText) die("a single read is larger than the batch size; raise --batch-bases");
        }
    }

    // MDBG_TRACE: what was inflated on the device, once the last slab is out
    void trace_totals() {
        if (!getenv("MDBG_TRACE")) return;
        if (!plan.gzips.empty())
            fprintf(stderr, "[mdbg_tool] device parse: %llu chunk(s) of %zu gzip file(s) inflated on the device in %llu call(s), %llu slab(s)\n", (unsigned long long)gzChunks,
                    plan.gzips.size(), (unsigned long long)gzCalls, (unsigned long long)gzSlabs);
        if (!plan.bgzfs.empty())
            fprintf(stderr, "[mdbg_tool] device parse: %llu BGZF block(s) of %zu file(s) inflated on the device in %llu slab(s) (%llu block inflations: a slab's first block may "
                            "be the one its predecessor ended in)\n", (unsigned long long)bgzfBlocks, plan.bgzfs.size(), (unsigned long long)bgzfSlabs,
                    (unsigned long long)bgzfInflated);
    }
};
