"""Diagnostic: class 64's setup priority in the stamps build (tools/phase_stamps.py) -- setup
cycles of the raised robots and of their CU-mates, raised robots per CU, and in how many CUs
the raised robot was the CU's slowest.
  python tools/setup_priority_stamps.py [B] [gaits]
Slot 12 of a robot's stamp record says whether it was raised.  PRIO_SWITCH=1 groups by the key of
the temporary switch that measured the mechanism instead (bit 3 xor bit 8 of the workgroup id:
two raised robots per CU; workgroup ids of one parity share their XCDs' parity, so a parity
switch would raise whole CUs or none)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_stamps as ps  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    gaits = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else ("trot10",)
    slots, iters = ps.run_raw(B, 10, gaits, 1000, with_iters=True)
    ts = slots[:, :7]
    d = np.diff(ts, axis=1)
    setup = ts[:, 3] - ts[:, 0]
    tot = ts[:, 6] - ts[:, 0]
    w0 = slots[:, 16]   # wave 0: HW_ID, XCC_ID << 32, workgroup id << 40
    blk = w0 >> 40
    raised = slots[:, 12] != 0
    if os.environ.get("PRIO_SWITCH"):
        raised = (((blk >> 3) ^ (blk >> 8)) & 1).astype(bool)
    cu = (((w0 & 0xffffffff) >> 8) & 0xff) | (((w0 >> 32) & 15) << 8)
    cus = np.unique(cu)
    print(f"B={B} robots, {int(raised.sum())} raised, {len(cus)} CUs")
    print("raised robots per CU, histogram:", np.bincount(np.array([raised[cu == c].sum() for c in cus])).tolist())
    slow_cu = np.array([int(np.argmax(np.where(cu == c, tot, -1))) for c in cus])
    print("CUs whose slowest robot was raised:", int(raised[slow_cu].sum()), "of", len(cus))
    for name, sel in (("all", np.ones(len(blk), bool)), ("raised", raised), ("not raised", ~raised)):
        if sel.sum() == 0:
            continue
        print(f"  {name:12s} n {int(sel.sum()):5d} setup median {np.median(setup[sel]):8.0f} | inputs-g {np.median(d[sel, 0]):7.0f} "
              f"H tile {np.median(d[sel, 1]):7.0f} sweep {np.median(d[sel, 2]):7.0f} | active set median "
              f"{np.median(d[sel, 3]):8.0f} | total median {np.median(tot[sel]):8.0f} max {tot[sel].max():8.0f}")
    i = int(np.argmax(tot))
    print(f"slowest robot {i}: raised {bool(raised[i])} total {tot[i]} setup {setup[i]} phases {d[i, :5].tolist()} "
          f"iterations {iters[i]}")
    rt = slots[:, 7:9]
    print(f"launch span (first start to last end): {(rt[:, 1].max() - rt[:, 0].min()) * 0.01:.2f} us")


if __name__ == "__main__":
    main()
