// ordered_place.hpp -- where the pieces of a file go when they are finished out of order, and the loop that puts them there.
// No threads, no locking (the caller holds its own lock), no library.
#pragma once
#include <unistd.h>

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <map>

namespace mdbg_host {

// Items arrive by sequence number (0, 1, 2, ... each once) in any order, each with its size in bytes.  An item's place in the file is
// the sum of the sizes of all earlier items, so it is known as soon as every earlier item has been added: add() reports every item
// whose place its call settled, in sequence order, through placed(seq, offset).
class OrderedPlace {
    std::map<uint64_t, uint64_t> waiting_;       // added, an earlier item still missing: seq -> bytes
    uint64_t nextSeq_ = 0, nextOff_ = 0;         // items [0, nextSeq_) have their place; they are nextOff_ bytes together
public:
    template <typename Placed>
    void add(uint64_t seq, uint64_t bytes, Placed &&placed) {
        waiting_[seq] = bytes;
        for (auto it = waiting_.find(nextSeq_); it != waiting_.end(); it = waiting_.find(nextSeq_)) {
            const uint64_t at = nextOff_;
            nextOff_ += it->second;
            waiting_.erase(it);
            placed(nextSeq_++, at);
        }
    }
    uint64_t next_seq() const { return nextSeq_; }
    uint64_t end_offset() const { return nextOff_; }
    size_t waiting() const { return waiting_.size(); }
    uint64_t first_waiting() const { return waiting_.begin()->first; }       // (waiting() > 0)
};

// pwrite until every byte is in the file.  false: a write failed (errno says how); the caller words the message
inline bool pwrite_all(int fd, const void *data, size_t bytes, uint64_t at) {
    for (size_t done = 0; done < bytes;) {
        const ssize_t w = pwrite(fd, (const char *)data + done, bytes - done, (off_t)(at + done));
        if (w < 0) { if (errno == EINTR) continue; return false; }
        done += (size_t)w;
    }
    return true;
}

}  // namespace mdbg_host
