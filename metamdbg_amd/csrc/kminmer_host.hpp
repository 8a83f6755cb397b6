// kminmer_host.hpp -- the host functions that cross between the k-min-mer translation units: kminmer.hip (the passes over sequences),
// tables.hip (the table handle), shard.hip (the sharded passes), partition.hip (the key-partitioned first pass).  A kernel is launched
// only from the unit that defines it; what another unit needs of it is one of these.
#pragma once
#include "common.hpp"
#include "objects.hpp"
#include "table.hpp"
#include "kminmer_dev.hpp"

#include <functional>
#include <memory>

namespace mdbg {

// ---- kminmer.hip ------------------------------------------------------------------------------------------------------------------
// first global instance of every sequence (windows of k minimizers) and their number
struct InstIndex {
    DevBuf<uint64_t> off;   // n_reads + 1
    uint64_t total = 0;
};
int build_inst_index(mdbg_ctx *ctx, const mdbg_minimizers *m, uint32_t k, InstIndex &ix);
SeqView make_view(const mdbg_minimizers *m, const InstIndex &ix);
int check_seq(mdbg_ctx *ctx, const mdbg_minimizers *m, const char *who);

int alloc_rows(mdbg_ctx *ctx, mdbg_table *t, uint64_t n, bool vec);
void update_key_hint(mdbg_ctx *ctx, int kind, uint64_t distinct, uint64_t instances);

// whether a first pass over n_min minimizers goes to the partitioned pass (partition.hip) before the one table
inline bool first_pass_partitioned(const mdbg_ctx *ctx, uint64_t n_min) {
    return ctx->first_pass_mode == 2 || (ctx->first_pass_mode == 0 && n_min >= ctx->part_auto_min);
}

// The insert stage of a first pass: every instance of `sv` counted in an adaptive table (count_insert_kernel), its slot kept in inst_slot.
// hint_kind: whose key ratio sizes the table (0: mdbg_kminmer_count_first, 3: mdbg_shard_begin).
int count_instances(mdbg_ctx *ctx, const SeqView &sv, uint32_t k, int hint_kind, DeviceTable &tab, DevBuf<uint32_t> &inst_slot);

// The rescue pass over one read set against the counts in a table: per-read decision, row positions, total.
struct RescuePlan {
    DevBuf<uint8_t> cls;      // 2-bit count class per table slot
    DevBuf<uint32_t> cnt;
    DevBuf<uint64_t> pos;
    uint64_t cap = 0, total = 0;
};
int plan_rescue(mdbg_ctx *ctx, const DeviceTable &tab, const InstIndex &ix, uint32_t n_reads, const uint32_t *inst_slot, RescuePlan &p);
void launch_emit_rescued(mdbg_ctx *ctx, const SeqView &sv, uint32_t k, const uint32_t *inst_slot, const RescuePlan &p, const RowOut &ro, uint64_t row_base);

// flag[s] = 1 for every occupied slot of `tab` (allocated here; untimed): the tables of which every key is a row
int flag_occupied_slots(mdbg_ctx *ctx, const DeviceTable &tab, DevBuf<uint32_t> &flag);

// From flags to the rows of a new table.  `flag` (tab.cap + TABLE_EXC_CAP entries) has just been filled by the caller; here the flags are
// prefix-scanned, their total read back, a table of k-min-mers allocated for total + extra rows and the flagged slots emitted as rows
// [0, total) (emit_slots_kernel; vectors from a / b when `vectors`).  The caller sets the statistics and synchronises.
//   timer        what the emit's interval is called for mdbg_timing_get, or null: untimed
//   extra_rows   (optional) runs once the total is known and says how many rows follow the table's own: the rescued ones
//   emit_extra   (optional) launches those rows behind the emit, inside the same interval
//   pos          the flags' prefix sums, which the emit in flight reads: `how` outlives the caller's synchronise
struct FlaggedRows {
    const char *timer = nullptr;
    std::function<int(uint64_t n_rows, uint64_t &extra)> extra_rows;
    std::function<void(const RowOut &ro, uint64_t n_rows)> emit_extra;
    DevBuf<uint64_t> pos;
};
int rows_from_flags(mdbg_ctx *ctx, const DeviceTable &tab, const DevBuf<uint32_t> &flag, uint32_t k, const SeqView &a, const SeqView &b, bool vectors,
                    FlaggedRows &how, std::unique_ptr<mdbg_table> &out);

// the look-up view of a previous table (built from its rows when it has none: abundance 1 skipped)
int prev_view(mdbg_ctx *ctx, const mdbg_table *prev, TableView &pv);

// ---- tables.hip -------------------------------------------------------------------------------------------------------------------
// build a lookup DeviceTable from the rows of `t` (abundance == 1 skipped as loadRefinedAbundances does, when skip_one)
int ensure_lookup(mdbg_ctx *ctx, mdbg_table *t, bool skip_one);

}  // namespace mdbg
