"""A numpy restatement of the bound loop's selection rule: how often does a selection refine, how
often does its winner hold an exact score from memory, and how large a cache of committed refines serves those winners?

    python tools/refine_model.py [--T 65536] [--K 256] [--W 64] [--L0 256] [--signals 1] [--kinds planted,noise]

Exact scores are float64 matrix products.  The bounds are the real formulas (csrc/hscmp_bound.h): one product per tap,
max_k |xh . dh_k| (1 + 2^-20) + kBoundEps1 ||xh_win|| cmax over the bf16-rounded window and dictionary; three products,
exact (1 + 2^-20) + 2^-13 ||x_win|| cmax.  Windows are zero padded at both passes (the engine's loop reflects at the signal
ends: a handful of rows per signal), weights are not modelled, and the products are summed in float64.  The selection is the
engine's: the leading position is refined while it holds a bound; the winner is applied and the rows p - (W-1) .. p + (W-1)
become bounds again.  The cache model keeps the most recent committed refines that did not win, drops an entry when an atom
lands within W - 1 of it, and counts a hit when the winner from memory is among the newest n entries.

On bench.py's own inputs (config 2: dictionary seed 2, signal 0) with the engine's bounds before the loop's one-product tile,
--init 1 --loop 3, the model gives 1.000 refines per selection on planted and 1.340 on noise: the two figures of
profiles/bound_one_product_stamps.txt (262 / 262 and 343 / 256 on the GPU).  With --init 1 --loop 1 (the default) it gives
1.000 and 1.43, and 64 entries serve every from-memory winner of both inputs (32 entries: about half of the noise ones)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS3 = 2.0 ** -13
EPS1 = 2.0 ** -7 * (1.0 + 2.0 ** -6)
CACHE_SIZES = (4, 8, 16, 32, 64)


def bf16(v):
    """bf16 round to nearest even of float32 values, as float32 (bf16_rn_bits)"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


class Model(object):
    def __init__(self, D):
        self.D = np.asarray(D, dtype=np.float32)
        self.K, self.W = self.D.shape
        self.D64 = self.D.astype(np.float64)
        self.Dh = bf16(self.D).astype(np.float64)
        self.cmax = float(np.sqrt((self.D64 ** 2).sum(1)).max())
        self.min_margin = np.inf                                # min over every bound formed of ub - exact

    def rows(self, r, t0, t1, products):
        """exact scores, bounds and coefficients of positions t0 .. t1-1 (window t .. t+W-1, zero padded)"""
        T, W = r.shape[0], self.W
        pad = np.concatenate([r[t0:min(T, t1 + W - 1)], np.zeros(max(0, t1 + W - 1 - T))])
        win = np.lib.stride_tricks.sliding_window_view(pad, W)[: t1 - t0]
        c = win @ self.D64.T
        ex = np.abs(c).max(1)
        if products == 3:
            ub = ex * (1 + 2.0 ** -20) + EPS3 * np.sqrt((win ** 2).sum(1)) * self.cmax
        else:
            wh = bf16(win.astype(np.float32)).astype(np.float64)
            ub = np.abs(wh @ self.Dh.T).max(1) * (1 + 2.0 ** -20) + EPS1 * np.sqrt((wh ** 2).sum(1)) * self.cmax
        self.min_margin = min(self.min_margin, float((ub - ex).min()))
        return ex, ub, c

    def run(self, x, L0, init_products=1, loop_products=1):
        """L0 selections on signal x.  Returns (refines per selection, winners from memory per selection,
        {cache size: hit rate among the winners from memory})."""
        T, W = x.shape[0], self.W
        r = x.astype(np.float64).copy()
        ex = np.empty(T)
        ub = np.empty(T)
        for t0 in range(0, T, 4096):
            t1 = min(T, t0 + 4096)
            ex[t0:t1], ub[t0:t1], _ = self.rows(r, t0, t1, init_products)
        cur = ub.copy()
        is_bound = np.ones(T, bool)
        refines = from_memory = 0
        cache = []
        hits = {n: 0 for n in CACHE_SIZES}
        for _ in range(L0):
            new = []
            while True:
                t = int(np.argmax(cur))
                if not is_bound[t]:
                    break
                cur[t] = ex[t]
                is_bound[t] = False
                refines += 1
                new.append(t)
            if t not in new:                                    # the winner's exact score was committed by an earlier selection
                from_memory += 1
                for n in hits:
                    hits[n] += t in cache[-n:]
            cache = [q for q in cache + [q for q in new if q != t] if abs(q - t) > W - 1]
            _, _, c = self.rows(r, t, t + 1, 3)
            k = int(np.argmax(np.abs(c[0])))
            n = min(W, T - t)
            r[t:t + n] -= c[0, k] * self.D64[k, :n]
            a, b = max(0, t - (W - 1)), min(T, t + W)
            ex[a:b], cur[a:b], _ = self.rows(r, a, b, loop_products)
            is_bound[a:b] = True
        return refines / L0, from_memory / L0, {n: h / max(1, from_memory) for n, h in hits.items()}


def main():
    import hsc_amd.synth as synth
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--T', type=int, default=65536)
    ap.add_argument('--K', type=int, default=256)
    ap.add_argument('--W', type=int, default=64)
    ap.add_argument('--L0', type=int, default=256)
    ap.add_argument('--signals', type=int, default=1)
    ap.add_argument('--init', type=int, default=1, choices=(1, 3), help='products per tap of the initial bound pass')
    ap.add_argument('--loop', type=int, default=1, choices=(1, 3), help='products per tap of the loop tile')
    ap.add_argument('--kinds', default='planted,noise')
    ap.add_argument('--seed', type=int, default=2)
    a = ap.parse_args()
    D = synth.make_dictionary(a.K, a.W, seed=a.seed)
    for kind in a.kinds.split(','):
        for i in range(a.signals):
            m = Model(D)
            x = np.asarray(synth.make_signal(D, a.T, i, kind=kind, nb_atoms=a.L0, seed=a.seed), dtype=np.float32).reshape(-1)
            per_sel, mem, rate = m.run(x, a.L0, a.init, a.loop)
            print('%s signal %d, init %d / loop %d: refines per selection %.3f, winners from memory per selection %.3f, '
                  'cache hit rate by entries %s, min(ub - exact) %.3g'
                  % (kind, i, a.init, a.loop, per_sel, mem, ' '.join('%d: %.0f %%' % (n, 100 * v) for n, v in rate.items()), m.min_margin),
                  flush=True)


if __name__ == '__main__':
    main()
