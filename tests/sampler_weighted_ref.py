"""Host restatement of amid_sample_negatives_weighted_i64 (amid_amd/csrc/sampling.hip), integer for integer what the kernel writes.
Same structure as oracle.sample_negatives_ref, with the popularity-weighted draw in place of the uniform one."""
import numpy as np

from oracle.amid_oracle import philox4x32

SITE_NEG_W = 0x4E57      # the weighted sampler's own RNG site (the uniform sampler keeps 0x4E45)


def weighted_candidates(pool: np.ndarray, cum: np.ndarray, r: int, round0: int, n_rounds: int, seed: int, epoch: int) -> np.ndarray:
    """The candidates row r sees in rounds [round0, round0 + n_rounds), in (round, lane) order, 64 per round.  The one of (round, lane)
    comes from Philox call (r << 20) | (round << 6) | lane at site SITE_NEG_W, step word = epoch: r64 = (x << 32) | y of its first two
    words, t = (r64 * total) >> 64 with total = cum[-1] (the 128-bit product in Python integers), and the candidate is pool[j] for the
    first j with cum[j] > t."""
    idx = (np.uint64(r) << np.uint64(20)) | np.arange(round0 * 64, (round0 + n_rounds) * 64, dtype=np.uint64)
    ctr = np.stack([
        (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32),
        (idx >> np.uint64(32)).astype(np.uint32),
        np.full(idx.size, SITE_NEG_W, dtype=np.uint32),
        np.full(idx.size, epoch & 0xFFFFFFFF, dtype=np.uint32),
    ], axis=1)
    words = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    total = int(cum[-1])
    t = np.array([(((int(x) << 32) | int(y)) * total) >> 64 for x, y in zip(words[:, 0].tolist(), words[:, 1].tolist())], dtype=np.int64)
    return pool[np.searchsorted(cum, t, side="right")]


def sample_negatives_weighted_ref(pool_d1, cum_d1, pool_d2, cum_d2, own_items, own_off, domain_id, k: int, seed: int, epoch: int,
                                  max_rounds: int = 4096, rounds_out=None) -> np.ndarray:
    """-> int64 [N, k].  Row r reads its stream of weighted candidates (weighted_candidates; domain_id[r] != 0 selects pool_d2 / cum_d2)
    and keeps, in stream order, the first k that are neither in its own list own_items[own_off[r]:own_off[r + 1]] nor kept already.  A
    row still short after max_rounds rounds gets -1 in slot 0; what it kept stays in the slots behind it and the slots never reached
    stay 0.  rounds_out: an optional list that receives, per row, the number of rounds the row consumed (max_rounds if it fell short)."""
    pools = (np.asarray(pool_d1, dtype=np.int64), np.asarray(pool_d2, dtype=np.int64))
    cums = (np.asarray(cum_d1, dtype=np.int64), np.asarray(cum_d2, dtype=np.int64))
    own_items, own_off = np.asarray(own_items, dtype=np.int64), np.asarray(own_off, dtype=np.int64)
    domain_id = np.asarray(domain_id)
    out = np.zeros((len(domain_id), k), dtype=np.int64)
    for r in range(len(domain_id)):
        d = int(domain_id[r] != 0)
        own = set(own_items[own_off[r]:own_off[r + 1]].tolist())
        kept: list = []
        seen = set()
        done, chunk, used = 0, 1, max_rounds     # rounds are drawn in growing chunks: most rows need one round, an exhausted one all
        while len(kept) < k and done < max_rounds:
            chunk = min(chunk, max_rounds - done)
            c = weighted_candidates(pools[d], cums[d], r, done, chunk, seed, epoch).tolist()
            for i, v in enumerate(c):
                if v not in own and v not in seen:
                    seen.add(v)
                    kept.append(v)
                    if len(kept) == k:
                        used = done + i // 64 + 1
                        break
            done += chunk
            chunk = min(2 * chunk, 256)
        out[r, :len(kept)] = kept
        if len(kept) < k:
            out[r, 0] = -1
        if rounds_out is not None:
            rounds_out.append(used)
    return out
