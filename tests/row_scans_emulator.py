"""numpy emulation of the row-scan form of the neighbour-form step (plan_fused.cpp, row_scans), driven by the plan's tables
like tests/fused_emulator.py, whose stages it rearranges:

  fused_tails   x tails as before; the combined rows of the y tails ALSO go through the tile-local x scans (zero carries)
  xscan_rows    (the step keeps its name) only tau[ty][tx][j*K+r][q][o]: the H_y contraction of the completed x carry strips
                entering the tile, formed from the RAW neighbour tails, c_0(t) = tau_0(t), c_1(t) = tau_1(t) + W_v(t)[0->1] tau_0(t-1)
  fused_pass2   completes the x carries it loads the same way; adds the residual sum_q tau[q] . G_vx[q] to each of the three
                y tails it loads (tile ty-1 scan 0, tile ty scan 0, tile ty+1 scan 1), then chains the anticausal one on its own
                causal tail with W_y

Whole 256 x TY tiles, a causal scan followed by an anticausal one in x and in y.  round_f32: every stored tail, row and tau
is rounded to f32, as the buffers between the launches hold them.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from fused_emulator import FusedEmu, TX
from tiled_emulator import scan_tile


class RowScansEmu(FusedEmu):
    def __init__(self, plan, scans, clamped, round_f32=False):
        super().__init__(plan, scans, clamped)
        self.round_f32 = round_f32
        assert [c for c, _ in self.xs] == [True, False] and [c for c, _ in self.ys] == [True, False]

    def _st(self, a):
        return np.asarray(a, dtype=np.float32).astype(np.float64) if self.round_f32 else np.asarray(a, dtype=np.float64)

    def run(self, img):
        img = np.asarray(img, dtype=np.float64)
        NY, NX = img.shape
        K, TY, clamped = self.K, self.TY, self.clamped
        assert NX % TX == 0 and NY % TY == 0, "the row-scan form takes whole tiles"
        MX, MY = NX // TX, NY // TY
        vxof = lambda tx: (1 if tx == 0 else 0) | (2 if tx == MX - 1 else 0)
        vyof = lambda ty: (1 if ty == 0 else 0) | (2 if ty == MY - 1 else 0)
        xfirst = lambda s, tx: tx == 0 if s == 0 else tx == MX - 1
        yfirst = lambda j, ty: ty == 0 if j == 0 else ty == MY - 1
        rows_of = lambda ty: slice(ty * TY, (ty + 1) * TY)
        cols_of = lambda tx: slice(tx * TX, (tx + 1) * TX)

        # ---- pass 1: x tails; combined rows, tile-locally scanned along x ----
        xt = np.zeros((2, MX, K, NY))
        yt = np.zeros((2, MY, K, NX))
        for ty in range(MY):
            for tx in range(MX):
                t = img[rows_of(ty), cols_of(tx)]
                for s in range(2):
                    for r in range(K):
                        xt[s, tx, r, rows_of(ty)] = self._st(t @ self.Hx[vxof(tx), s, r])
                rows = np.stack([self.Hy[vyof(ty), j, r] @ t for j in range(2) for r in range(K)])
                for s in range(2):
                    rows = self.xphase(rows, s, None, clamped and xfirst(s, tx))
                for j in range(2):
                    for r in range(K):
                        yt[j, ty, r, cols_of(tx)] = self._st(rows[j * K + r])

        def xcarry(s, tx, ty):
            """the completed x carry of scan s entering tile (tx, ty), [K, TY], from the raw tails; None at the border"""
            if xfirst(s, tx):
                return None
            if s == 0:
                return xt[0, tx - 1][:, rows_of(ty)]
            return xt[1, tx + 1][:, rows_of(ty)] + self.Wx[vxof(tx + 1), 0, 1] @ xt[0, tx][:, rows_of(ty)]

        # ---- the middle launch: tau only ----
        tau = np.zeros((MY, MX, 2 * K, 2, K))
        for ty in range(MY):
            for tx in range(MX):
                for q in range(2):
                    c = xcarry(q, tx, ty)
                    if c is None:
                        continue
                    for j in range(2):
                        for r in range(K):
                            tau[ty, tx, j * K + r, q] = self._st(c @ self.Hy[vyof(ty), j, r])

        def ytail(j, ty, tx):
            """y tail j of tile (tx, ty) with the residual, [K, 256]"""
            out = yt[j, ty][:, cols_of(tx)].copy()
            for r in range(K):
                for q in range(2):
                    out[r] = out[r] + tau[ty, tx, j * K + r, q] @ self.G[vxof(tx), q]
            return out

        # ---- pass 2 ----
        out = np.empty_like(img)
        for ty in range(MY):
            for tx in range(MX):
                t = img[rows_of(ty), cols_of(tx)].copy()
                for s in range(2):
                    t = self.xphase(t, s, xcarry(s, tx, ty), clamped and xfirst(s, tx))
                cy = [None, None]
                if ty > 0:
                    cy[0] = ytail(0, ty - 1, tx)
                if ty < MY - 1:
                    cy[1] = ytail(1, ty + 1, tx) + self.Wy[vyof(ty + 1), 0, 1] @ ytail(0, ty, tx)
                for j in range(2):
                    v = np.ascontiguousarray(t.T)
                    b, a = self.yc[j]
                    scan_tile(v, j == 0, b, a, K, clamped and yfirst(j, ty), None if cy[j] is None else [cy[j][r] for r in range(K)])
                    t = v.T.copy()
                out[rows_of(ty), cols_of(tx)] = t
        return out
