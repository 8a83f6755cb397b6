"""Regenerates tests/golden/read_mapper: seeded reads in minimizer space and what the REFERENCE's read mapper computes for them -- the
sorted index of ReadFunctor + sortParallel, the anchors of AlignReadsLowDensityFunctor::operator() and the Chain2 of chainAnchors for
every (query, reference read) group -- by mapper_ref.cpp, which is compiled here against the reference's sources with the flags of
oracle/Makefile.  No test runs this; only the data it wrote is read by tests/test_read_mapper_model.py and tests/test_gpu_read_mapper.py.

    python tests/golden/read_mapper/make_fixture.py --ref <path of the reference>

The reads: a few random "genomes" of u32 minimizers with positions 20 - 60 apart, sampled into about 300 reads of 2 - 250 minimizers, half
of them on the reverse strand, positions jittered, 2 % of the minimizers substituted and 2 % dropped.  The genomes carry tandem repeats
(a, b, a, b ...: the pair (a, b) followed by (b, a)), runs of one minimizer (windows with a == b), short segments shared between genomes
at other spacings (anchors that do not chain) and inverted copies (pairs that mix both strands); a few reads are placed on purpose: two
that overlap over 250 minimizers, reads that start inside a long tandem repeat another read spans (the true predecessor lies further
back than the band), reads of 0, 1, 2 and 9 minimizers.

One configuration per band: 62 (the default 2500 * 0.025), 5 and 100.  The conditions on the selection are asserted below (conditions,
not measurements; manifest.json records the counts) -- seeds are tried in order until the reference's output meets them.

Files: manifest.json, <name>.npz --
  read_offsets, minimizers, positions              the reads
  index_pair / _read / _position / _index / _reversed      the reference's sorted index, in its order
  query_anchors (per read), anchor_ref_read / _ref_position / _ref_index / _query_position / _query_index / _reversed
                                                   every anchor (min_anchors = 1), in the reference's order
  pair_query, pair_ref_read, pair_anchors, pair_score      every (query, reference read) group; pair_anchors < 3: processAnchors drops it;
                                                   pair_score 0: no chain
  chain_n_matches / _query_reversed / _n_diff_query / _n_diff_reference / _query_start / _query_end / _reference_start / _reference_end
                                                   Chain2's fields per group (0 where there is no chain)
  match_offsets (groups + 1), matches              _queryAnchorPositions
The arrays manifest.json lists under delta_coded are stored as first differences (tests/mapper_model.py, load_fixture, sums them up)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
SPANS = os.path.join(os.path.dirname(HERE), "kminmer_spans")
CONFIGS = (("band62", 62), ("band5", 5), ("band100", 100))
# stored as first differences (int32), which deflate far better; mapper_model.load_fixture sums them up again
DELTA_CODED = ("positions", "index_position", "index_index", "anchor_ref_position", "anchor_ref_index", "anchor_query_position", "anchor_query_index")
CHAIN_FIELDS = ("n_matches", "query_reversed", "n_diff_query", "n_diff_reference", "query_start", "query_end", "reference_start", "reference_end")


def draw_genomes(rng, n_genomes=3, length=600):
    """Per genome (minimizers, gaps): gaps[i] is the distance from minimizer i to minimizer i + 1."""
    fresh = lambda n: rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    shared = [(fresh(6), rng.integers(20, 60, 6)) for _ in range(4)]       # segments every genome carries, each copy at its own spacing
    genomes = []
    for _ in range(n_genomes):
        parts, gaps = [], []

        def add(m, g):
            parts.append(np.asarray(m, np.uint32))
            gaps.append(np.asarray(g, np.int64))

        while sum(len(p) for p in parts) < length:
            kind = rng.random()
            if kind < 0.70:
                n = int(rng.integers(20, 80))
                add(fresh(n), rng.integers(20, 60, n))
            elif kind < 0.78:                                            # a, b, a, b ...: the pair (a, b), then (b, a)
                a, b = fresh(2)
                n = int(rng.integers(2, 9))
                add(np.tile([a, b], n), np.full(2 * n, int(rng.integers(20, 60))))
            elif kind < 0.82:                                            # a run of one minimizer: windows with a == b
                n = int(rng.integers(2, 6))
                add(np.full(n, fresh(1)[0]), rng.integers(20, 60, n))
            elif kind < 0.92:                                            # a shared segment, stretched: its anchors are too far off the diagonal to chain
                m, g = shared[int(rng.integers(0, len(shared)))]
                add(m, g + int(rng.integers(0, 12)) * 130)
            elif parts:                                                  # an inverted copy of something earlier
                k = int(rng.integers(0, len(parts)))
                add(parts[k][::-1][:12], gaps[k][::-1][:12])
        # one long tandem repeat: a read that starts inside it meets a read that spans it (draw_reads)
        a, b = fresh(2)
        add(np.tile([a, b], 60 if not genomes else 4), np.full(120 if not genomes else 8, 40))
        add(fresh(60), rng.integers(20, 60, 60))
        genomes.append((np.concatenate(parts), np.concatenate(gaps)))
    return genomes


def sample_read(rng, genome, start, n, reverse, jitter=3, p_sub=0.02, p_drop=0.02):
    m, g = genome
    n = min(n, len(m) - start)
    mins = m[start:start + n].copy()
    gaps = g[start:start + n].copy()
    if n:
        gaps = gaps + rng.integers(-jitter, jitter + 1, n) if jitter else gaps
        sub = rng.random(n) < p_sub
        mins[sub] = rng.integers(1, 1 << 32, int(sub.sum()), dtype=np.uint64).astype(np.uint32)
    pos = int(rng.integers(0, 200)) + np.concatenate([[0], np.cumsum(gaps[:-1])]) if n else np.zeros(0, np.int64)
    keep = rng.random(n) >= p_drop
    mins, pos = mins[keep], pos[keep]
    if reverse and len(pos):
        mins, pos = mins[::-1], (pos[-1] + int(rng.integers(0, 200))) - pos[::-1]
    return mins.astype(np.uint32), pos.astype(np.uint32)


def draw_reads(seed: int):
    rng = np.random.default_rng(seed)
    genomes = draw_genomes(rng)
    reads = []
    for _ in range(250):                                                 # (none of these reaches a genome's long tandem repeat: its grids of anchors
        gm = genomes[int(rng.integers(0, len(genomes)))]                 # between every two reads that span it would be most of the fixture)
        u = rng.random()
        n = int(rng.integers(2, 12)) if u < 0.55 else int(rng.integers(12, 34)) if u < 0.99 else int(rng.integers(150, 251))
        start = int(rng.integers(0, len(gm[0]) - 200))       # (the other genomes' tails: 68)
        reads.append(sample_read(rng, gm, start, min(n, len(gm[0]) - 200 - start), rng.random() < 0.5, jitter=0 if rng.random() < 0.3 else 3))
    for gm in genomes[:1]:
        rep = len(gm[0]) - 180                                           # where the long tandem repeat starts
        reads.append(sample_read(rng, gm, rep - 20, 200, False, jitter=0, p_sub=0, p_drop=0))      # spans it
        reads.append(sample_read(rng, gm, rep + 112, 60, False, jitter=0, p_sub=0, p_drop=0))      # starts inside it, 8 windows before its end
        reads.append(sample_read(rng, gm, rep + 110, 60, True, jitter=1, p_sub=0, p_drop=0))
        reads.append(sample_read(rng, gm, rep + 108, 50, False, jitter=1, p_sub=0, p_drop=0))
        reads.append(sample_read(rng, gm, rep + 114, 40, True, jitter=0, p_sub=0, p_drop=0))
    # twelve reads that share one segment of six minimizers, each at its own spacing: five anchors a pair, none follows another
    fresh = lambda n: rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    seg, seg_gaps = fresh(6), rng.integers(20, 60, 6)
    for k in range(12):
        m = np.concatenate([fresh(5), seg, fresh(5)])
        g = np.concatenate([rng.integers(20, 60, 5), seg_gaps + 130 * k, rng.integers(20, 60, 5)])
        reads.append(sample_read(rng, (m, g), 0, 16, k % 2 == 1, jitter=0, p_sub=0, p_drop=0))
    reads.append(sample_read(rng, genomes[0], 100, 250, False))         # two reads over the same 250 minimizers
    reads.append(sample_read(rng, genomes[0], 100, 250, True))
    for n in (0, 1, 2, 9):
        reads.append(sample_read(rng, genomes[1], 300, n, False, p_drop=0))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def run_reference(exe: str, reads, band: int, tmp: str) -> dict:
    text = [str(len(reads))]
    for m, p in reads:
        text.append(" ".join([str(len(m))] + [f"{int(a)} {int(b)}" for a, b in zip(m, p)]))
    out = subprocess.run([exe, str(band), tmp], input=("\n".join(text) + "\n").encode(), capture_output=True, check=True).stdout.decode()
    index, anchors, q_anchors, pairs, chains, matches, match_offsets = [], [], [], [], [], [], [0]
    seconds = 0.0
    query = -1
    for line in out.splitlines():
        tag, *f = line.split()
        if tag == "I":
            index.append([int(x) for x in f])
        elif tag == "Q":
            query = int(f[0])
            assert query == len(q_anchors)
            q_anchors.append(int(f[1]))
        elif tag == "A":
            anchors.append([int(x) for x in f])
        elif tag == "P":
            pairs.append([query, int(f[0]), int(f[1]), int(f[2])])
            chains.append([0] * 8)
            match_offsets.append(len(matches))
        elif tag == "C":
            v = [int(x) for x in f]
            chains[-1] = v[:8]
            assert v[8] == len(v) - 9
            matches.extend(v[9:])
            match_offsets[-1] = len(matches)
        elif tag == "T":
            seconds = float(f[0])
    index = np.array(index, dtype=np.uint64).reshape(-1, 5)
    anchors = np.array(anchors, dtype=np.int64).reshape(-1, 6)
    pairs = np.array(pairs, dtype=np.int64).reshape(-1, 4)
    chains = np.array(chains, dtype=np.int64).reshape(-1, 8)
    offsets = np.concatenate([[0], np.cumsum([len(m) for m, _ in reads])]).astype(np.uint64)
    cat = lambda k: np.concatenate([r[k] for r in reads]).astype(np.uint32)
    data = dict(read_offsets=offsets, minimizers=cat(0), positions=cat(1),
                index_pair=index[:, 0], index_read=index[:, 1].astype(np.uint32), index_position=index[:, 2].astype(np.uint32),
                index_index=index[:, 3].astype(np.uint32), index_reversed=index[:, 4].astype(np.uint8),
                query_anchors=np.array(q_anchors, np.uint32),
                anchor_ref_read=anchors[:, 0].astype(np.uint32), anchor_ref_position=anchors[:, 1].astype(np.uint32), anchor_ref_index=anchors[:, 2].astype(np.uint32),
                anchor_query_position=anchors[:, 3].astype(np.uint32), anchor_query_index=anchors[:, 4].astype(np.uint32), anchor_reversed=anchors[:, 5].astype(np.uint8),
                pair_query=pairs[:, 0].astype(np.uint32), pair_ref_read=pairs[:, 1].astype(np.uint32), pair_anchors=pairs[:, 2].astype(np.uint32),
                pair_score=pairs[:, 3].astype(np.int32), match_offsets=np.array(match_offsets, np.uint64), matches=np.array(matches, np.uint32))
    data.update({"chain_" + name: chains[:, c] for c, name in enumerate(CHAIN_FIELDS)})
    return data, seconds


def conditions(data: dict, band: int) -> dict:
    """The conditions on the selection (asserted here and again by tests/test_read_mapper_model.py): not measurements."""
    sys.path.insert(0, os.path.dirname(TESTS))
    from tests import mapper_model as mm
    found = data["pair_score"] != 0
    lens = np.diff(data["read_offsets"].astype(np.int64))
    pa = data["pair_anchors"].astype(np.int64)
    ao = np.concatenate([[0], np.cumsum(pa)])
    mixed = sum(1 for p in range(len(pa)) if len(set(data["anchor_reversed"][ao[p]:ao[p + 1]].tolist())) == 2)
    w = mm.windows(data["minimizers"], data["read_offsets"], data["positions"])
    short_hit = 0                                      # queries below 10 minimizers with a window whose pair another read has too
    for r in np.flatnonzero(lens < mm.MIN_QUERY_MINIMIZERS):
        mine = w["pair"][w["local_read"] == r]
        short_hit += bool(np.isin(data["index_pair"][data["index_read"] != r], mine).any())
    ix_runs = {}
    for pair, read in zip(data["index_pair"].tolist(), data["index_read"].tolist()):
        ix_runs.setdefault(pair, []).append(read)
    self_hit = len({r for reads in ix_runs.values() for r in reads if reads.count(r) > 1})      # reads with two windows of one pair: they meet their own entries twice
    c = dict(chains_query_reversed=int((found & (data["chain_query_reversed"] == 1)).sum()), chains_query_forward=int((found & (data["chain_query_reversed"] == 0)).sum()),
             pairs_below_3=int((pa < 3).sum()), pairs_3_up_without_chain=int(((pa >= 3) & ~found).sum()), pairs_mixing_strands=int(mixed),
             short_queries_hitting=short_hit, reads_hitting_own_windows=int(self_hit), longest_pair=int(pa.max()))
    assert c["chains_query_reversed"] >= 50 and c["chains_query_forward"] >= 50, c
    assert c["pairs_below_3"] >= 20 and c["pairs_3_up_without_chain"] >= 20 and c["pairs_mixing_strands"] >= 10, c
    assert c["short_queries_hitting"] >= 5 and c["reads_hitting_own_windows"] >= 5 and c["longest_pair"] > band + 64, c
    # ... and, by the numpy model once it equals the reference on the whole fixture:
    ix = mm.build_index(data["minimizers"], data["read_offsets"], data["positions"])
    an = mm.anchors(ix, data["minimizers"], data["read_offsets"], data["positions"], min_anchors=1)
    assert np.array_equal(an["ref_position"], data["anchor_ref_position"]) and np.array_equal(an["query_index"], data["anchor_query_index"])
    stats = {}
    ch = mm.chains(an, band, stats)
    assert np.array_equal(ch["chains"]["score"], data["pair_score"]) and np.array_equal(ch["matches"], data["matches"]), "the model is not the reference"
    free = mm.chains(an, None)
    c.update(anchors_with_tied_predecessors=int(stats.get("pred_ties", 0)), pairs_with_tied_best=int(stats.get("end_ties", 0)),
             pairs_changed_by_the_band=int((free["chains"]["score"] != ch["chains"]["score"]).sum()))
    assert c["anchors_with_tied_predecessors"] >= 10 and c["pairs_with_tied_best"] >= 3 and c["pairs_changed_by_the_band"] >= 3, c
    return c


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (holds src/Commons.hpp)")
    ap.add_argument("--first-seed", type=int, default=7100)
    args = ap.parse_args()
    limit = max(os.path.getsize(os.path.join(SPANS, f)) for f in os.listdir(SPANS))
    manifest = dict(delta_coded=list(DELTA_CODED), configs=[])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mapper_ref")
        subprocess.run(["g++", "-std=gnu++20", "-O2", "-w", "-fopenmp", "-I" + os.path.join(args.ref, "src"), "-I" + args.ref,
                        os.path.join(HERE, "mapper_ref.cpp"), os.path.join(args.ref, "src", "utils", "MurmurHash3.cpp"), "-lz", "-o", exe], check=True)
        seed = args.first_seed
        for name, band in CONFIGS:
            while True:
                reads = draw_reads(seed)
                data, seconds = run_reference(exe, reads, band, tmp)
                try:
                    found = conditions(data, band)
                    break
                except AssertionError as e:
                    print(name, "seed", seed, "does not meet the conditions:", e)
                    seed += 1
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, **{k: (np.diff(v.astype(np.int64), prepend=0).astype(np.int32) if k in DELTA_CODED else v) for k, v in data.items()})
            assert os.path.getsize(path) <= limit, (os.path.getsize(path), limit)
            manifest["configs"].append(dict(name=name, band=band, seed=seed, n_reads=len(reads), n_minimizers=int(data["read_offsets"][-1]),
                                            n_index_entries=len(data["index_pair"]), n_anchors=len(data["anchor_ref_read"]), n_pairs=len(data["pair_query"]),
                                            n_chains=int((data["pair_score"] != 0).sum()), n_matches=len(data["matches"]), reference_seconds=round(seconds, 4), **found))
            print(name, "seed", seed, os.path.getsize(path), "bytes of fixture", manifest["configs"][-1])
            seed += 1
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
