"""Device side of the offline evaluation sweep's tests (tests/test_sweep.py, tests/test_sweep_windows.py): rs_polya_coords on a
batch of reads at odd sample offsets, with a caller's lengths, cut and workspace, and the comparison with the numpy mirror of
tests/sweep_ref.py."""
import numpy as np
import torch

from riser_amd import _native as nv
from tests import sweep_ref as R


def device_scan(dev, reads, res, thr, lens=None, max_len=None, ws=None, table=False):
    """rs_polya_coords with every read at an ODD sample offset (a filler of 32767 goes in front of a read that would start
    at an even one), `lens` in place of the true lengths, a caller's workspace -> (starts, ends) on the host; with `table`
    also the workspace's first rs_polya_coords_workspace_bytes as int32 [B, max_len // res, 2] = (window sum, 4 x MAD)."""
    parts, offs, pos = [], [], 0
    for r in reads:
        if pos % 2 == 0:
            parts.append(np.full(1, 32767, dtype=np.int16))
            pos += 1
        offs.append(pos)
        parts.append(np.asarray(r, dtype=np.int16))
        pos += len(r)
    parts.append(np.full(3, 32767, dtype=np.int16))
    true_lens = np.array([len(r) for r in reads], dtype=np.int32)
    lens = true_lens if lens is None else np.asarray(lens, dtype=np.int32)
    if max_len is None:
        max_len = int(max(int(lens.max()), 0))
    assert all(min(int(n), max_len) <= int(t) for n, t in zip(lens, true_lens)), "the test itself would read out of bounds"
    B = len(reads)
    sig = torch.from_numpy(np.concatenate(parts)).to(dev)
    off = torch.from_numpy(np.array(offs, dtype=np.int64)).to(dev)
    ln = torch.from_numpy(lens).to(dev)
    st = torch.full((B,), -7, dtype=torch.int32, device=dev)
    en = torch.full((B,), -7, dtype=torch.int32, device=dev)
    L = nv.lib()
    need = int(L.rs_polya_coords_workspace_bytes(B, max_len, res))
    if ws is None:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    nv.check(L.rs_polya_coords(sig.data_ptr(), off.data_ptr(), ln.data_ptr(), B, max_len, res, thr, st.data_ptr(), en.data_ptr(),
                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "rs_polya_coords")
    torch.cuda.synchronize(dev)
    if not table:
        return st.cpu().numpy(), en.cpu().numpy()
    pitch = max_len // res
    assert need == max(B * pitch, 1) * 8
    tab = ws[: B * pitch * 8].cpu().numpy().view(np.int32).reshape(B, pitch, 2)
    return st.cpu().numpy(), en.cpu().numpy(), tab


def assert_mirror(dev, reads, res, thr, **kw):
    st, en = device_scan(dev, reads, res, thr, **kw)
    lens = kw.get("lens")
    cut = kw.get("max_len")
    seen = []
    for i, r in enumerate(reads):
        n = len(r) if lens is None else max(int(lens[i]), 0)
        seen.append(r[: n if cut is None else min(n, cut)])
    wst, wen = R.polya_coords_batch(seen, res, thr)
    assert np.array_equal(st, wst) and np.array_equal(en, wen), (res, thr, st.tolist(), wst.tolist(), en.tolist(), wen.tolist())
    return st, en
