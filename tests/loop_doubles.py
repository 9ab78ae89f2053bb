"""CPU restatements of the elementwise HIP entries the sampler loop calls (include/mmgt_hip.h: mmgt_accumulate_window, mmgt_accumulate_windows,
mmgt_cfg_ddim_step), for the host-logic tests that run the loop over a CPU double of the operator.  Order-preserving as the kernels are: window by
window in list order, one fp32 add per target and window.  With weights the product is rounded before the add (torch has no fmaf); weights of 1
give the plain add either way."""


def _add_window(p5, pred_sum, counter, idx, weights, row0, bump):
    """p5 (rows, C, Fw, h, w) into CFG rows [row0, row0 + rows) at frames idx; counter collects the weights (1 per position without)"""
    i = idx.long()
    pred_sum[row0:row0 + p5.shape[0], :, i] += p5 if weights is None else weights.view(1, 1, -1, 1, 1) * p5
    if bump:
        counter[i] += 1 if weights is None else weights


def install(monkeypatch, hip_mod):
    """Puts the doubles in place of hip_mod's bindings through pytest's monkeypatch, so that the real ones are back for every later test of the
    session.  -> the call log of the two accumulations: one (form, rows, row0, weights given) per call, form "window" or "windows"."""
    log = []

    def accumulate_window(pred, pred_sum, counter, idx, C, rows=2, row0=0, bump_counter=True, weights=None):
        log.append(("window", rows, row0, weights is not None))
        fw = idx.numel()
        assert idx.dim() == 1 and pred.shape[0] == rows * fw
        p5 = pred[..., :C].reshape(rows, fw, pred.shape[1], pred.shape[2], C).permute(0, 4, 1, 2, 3)
        _add_window(p5, pred_sum, counter, idx, weights, row0, bump_counter)

    def accumulate_windows(pred, pred_sum, counter, idx, C, rows=2, row0=0, weights=None):
        log.append(("windows", rows, row0, weights is not None))
        nb, fw = idx.shape
        assert pred.shape[0] == rows * nb * fw
        p6 = pred[..., :C].reshape(rows, nb, fw, pred.shape[1], pred.shape[2], C)
        for k in range(nb):
            _add_window(p6[:, k].permute(0, 4, 1, 2, 3), pred_sum, counter, idx[k], weights, row0, True)

    def cfg_ddim_step(pred_sum, counter, latents, g, sa_t, sb_t, sa_p, sb_p):
        avg = pred_sum / counter.view(1, 1, -1, 1, 1)
        v = avg[0:1] + g * (avg[1:2] - avg[0:1])
        return sa_p * (sa_t * latents - sb_t * v) + sb_p * (sa_t * v + sb_t * latents)
    monkeypatch.setattr(hip_mod, "accumulate_window", accumulate_window)
    monkeypatch.setattr(hip_mod, "accumulate_windows", accumulate_windows)
    monkeypatch.setattr(hip_mod, "cfg_ddim_step", cfg_ddim_step)
    return log
