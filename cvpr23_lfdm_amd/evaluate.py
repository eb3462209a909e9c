"""Paired, full-reference evaluation on the device: what the reference's test scripts measure
(LFAE/test_flowautoenc_*.py: out_loss / warp_loss) plus per-frame L1, MSE / PSNR and SSIM in image space and the end-point / occlusion
error in latent-flow space, through ops.video_metrics / ops.flow_metrics (csrc/metrics.hip).  Nothing here copies a video to the host:
the per-frame tables are float64 tensors on the model's device, and nothing synchronises until a number is read: the accumulators are read
once, at the end, and the "summary" / "out_loss" / "warp_loss" entries of the comparison results are computed when first read.

    acc = MetricAccumulator()
    for real_vid, ref_img in loader:
        acc.update(compare_videos(model_out(ref_img), real_vid, mean=MEAN)["table"])
    print(acc.result())

FVD and other learned metrics are not here: they need networks this package does not ship.
"""
import math

import torch

from . import ops

__all__ = ["MetricAccumulator", "FlowAccumulator", "compare_videos", "compare_flows", "reference_loss", "lfae_reconstruction", "sample_against_real",
           "ab_compare", "interpolation_error"]


class _Result(dict):
    """A dict whose listed entries are computed - one device synchronisation - when they are first read with result[key]; until then
    they are not among its keys, so a loop that only takes the tables never waits for the device."""

    def __init__(self, eager, lazy):
        super().__init__(eager)
        self._lazy = dict(lazy)

    def __missing__(self, key):
        if key not in self._lazy:
            raise KeyError(key)
        self[key] = self._lazy.pop(key)()
        return self[key]


class MetricAccumulator:
    """Running float64 sums of per-frame metric tables, kept on the tables' device.  update() launches a few small kernels and does
    not synchronise; result() copies seven numbers once."""

    def __init__(self):
        self._sums = None          # [l1, mse, ssim, psnr over frames with mse > 0, number of such frames]
        self.frames = 0
        self.videos = 0

    def update(self, table):
        """table: (B, T, 3) float64 [l1, mse, ssim] per frame, as ops.video_metrics returns it."""
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float64 or table.dim() != 3 or table.shape[2] != 3:
            raise ValueError("MetricAccumulator.update: a (B, T, 3) float64 table, got %s %s"
                             % (getattr(table, "dtype", type(table)), tuple(getattr(table, "shape", ()))))
        rows = table.reshape(-1, 3)
        mse = rows[:, 1].contiguous()
        positive = mse > 0
        psnr = torch.where(positive, ops.psnr(mse), torch.zeros_like(mse))
        add = torch.cat((rows.sum(dim=0), psnr.sum().reshape(1), positive.sum().to(torch.float64).reshape(1)))
        self._sums = add if self._sums is None else self._sums + add
        self.frames += rows.shape[0]
        self.videos += table.shape[0]
        return self

    def result(self):
        """Plain floats: l1, mse, ssim (means over all frames), psnr (the mean of the per-frame PSNR over the frames with mse > 0; inf
        when there is none), identical_frames (the frames with mse == 0, which psnr leaves out), frames, videos, and l1_frame_sum (the
        sum of the per-frame l1, which reference_loss turns into the reference scripts' normalisation)."""
        if self._sums is None:
            raise RuntimeError("MetricAccumulator.result: nothing has been accumulated")
        l1, mse, ssim, psnr_sum, psnr_frames = self._sums.cpu().tolist()          # the one synchronisation
        n = float(self.frames)
        psnr_frames = int(round(psnr_frames))
        return dict(l1=l1 / n, mse=mse / n, ssim=ssim / n, psnr=psnr_sum / psnr_frames if psnr_frames else math.inf,
                    identical_frames=self.frames - psnr_frames, frames=self.frames, videos=self.videos, l1_frame_sum=l1)


def reference_loss(summary, channels=3):
    """out_loss / warp_loss as LFAE/test_flowautoenc_*.py prints them: the L1 SUM over every value of every frame divided by
    videos * H * W * 3 - not by the frame count, so it grows with the length of the videos.  From a "raw"-domain summary."""
    return summary["l1_frame_sum"] * channels / (3.0 * summary["videos"])


class FlowAccumulator:
    """MetricAccumulator's counterpart for ops.flow_metrics tables: two float64 sums on the device, update() does not synchronise."""

    def __init__(self):
        self._sums = None
        self.frames = 0
        self.videos = 0

    def update(self, table):
        """table: (B, T, 2) float64 [end-point error, occlusion error] per latent frame."""
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float64 or table.dim() != 3 or table.shape[2] != 2:
            raise ValueError("FlowAccumulator.update: a (B, T, 2) float64 table, got %s %s"
                             % (getattr(table, "dtype", type(table)), tuple(getattr(table, "shape", ()))))
        add = table.reshape(-1, 2).sum(dim=0)
        self._sums = add if self._sums is None else self._sums + add
        self.frames += table.shape[0] * table.shape[1]
        self.videos += table.shape[0]
        return self

    def result(self):
        """Plain numbers: epe, occlusion_error (means over all frames), frames, videos."""
        if self._sums is None:
            raise RuntimeError("FlowAccumulator.result: nothing has been accumulated")
        epe, occ = self._sums.cpu().tolist()          # the one synchronisation
        return dict(epe=epe / self.frames, occlusion_error=occ / self.frames, frames=self.frames, videos=self.videos)


def compare_videos(a, b, mean=(0, 0, 0), domain="unit"):
    """a against b, (B, C, T, H, W) fp32 each -> {"table": (B, T, 3) float64 [l1, mse, ssim], "psnr": (B, T) float64 (inf where the
    frames are equal), "summary": MetricAccumulator.result() of the table, computed when first read}.  mean / domain: ops.video_metrics."""
    table = ops.video_metrics(a, b, mean=mean, domain=domain)
    return _Result({"table": table, "psnr": ops.psnr(table[:, :, 1])}, {"summary": lambda: MetricAccumulator().update(table).result()})


def compare_flows(grid_a, grid_b, conf_a=None, conf_b=None):
    """-> {"table": (B, T, 2) float64 [end-point error, occlusion error] per latent frame, "summary": FlowAccumulator.result() of the
    table (their means, frames, videos), computed when first read}."""
    table = ops.flow_metrics(grid_a, grid_b, conf_a, conf_b)
    return _Result({"table": table}, {"summary": lambda: FlowAccumulator().update(table).result()})


def _frozen_lfae(model, real_vid, ref_img):
    if model.is_train:
        raise ValueError("evaluation runs the frozen LFAE pass of a model built with is_train=False")
    if real_vid.dim() != 5 or ref_img.dim() != 4 or real_vid.shape[0] != ref_img.shape[0]:
        raise ValueError("real_vid must be (B, 3, T, H, W) and ref_img (B, 3, H, W), got %s and %s"
                         % (tuple(real_vid.shape), tuple(ref_img.shape)))
    model.set_train_input(ref_img=ref_img, real_vid=real_vid, ref_text=None)
    with torch.no_grad():
        model.forward()
    return model.real_vid.float()


def lfae_reconstruction(model, real_vid, ref_img, mean=(0, 0, 0), domain="unit"):
    """The reference's test_flowautoenc_* measurement of one batch: every frame of real_vid reconstructed from ref_img through the
    frozen LFAE (FlowDiffusion.forward() of an is_train=False model), real_out_vid and real_warped_vid compared with real_vid.
    -> {"out": compare_videos(real_out_vid, real_vid, mean, domain), "warp": the same for real_warped_vid, "out_raw" / "warp_raw":
    the same in the "raw" domain, "out_loss" / "warp_loss": the reference's two numbers for this batch (reference_loss of the raw
    summaries), computed when first read}.  Feed the tables to MetricAccumulators to cover a data set."""
    real = _frozen_lfae(model, real_vid, ref_img)
    res = {"out": compare_videos(model.real_out_vid, real, mean, domain), "warp": compare_videos(model.real_warped_vid, real, mean, domain),
           "out_raw": compare_videos(model.real_out_vid, real, domain="raw", mean=(0,) * real.shape[1]),
           "warp_raw": compare_videos(model.real_warped_vid, real, domain="raw", mean=(0,) * real.shape[1])}
    channels = real.shape[1]
    return _Result(res, {"out_loss": lambda: reference_loss(res["out_raw"]["summary"], channels),
                         "warp_loss": lambda: reference_loss(res["warp_raw"]["summary"], channels)})


def sample_against_real(model, real_vid, mean=(0, 0, 0), domain="unit"):
    """After sample_one_video / sample_long_video from model.sample_img: the sampled video against the real one it should resemble.
    -> {"vs_real": sample_out_vid against real_vid, "vs_lfae": sample_out_vid against the LFAE's own reconstruction of real_vid from
    the same image (the best the diffusion model can reach), "lfae": that reconstruction against real_vid (compare_videos each),
    "flow": compare_flows of sample_vid_grid / sample_vid_conf against the pseudo ground truth real_vid_grid / real_vid_conf}."""
    if model.sample_out_vid is None:
        raise RuntimeError("sample_against_real: nothing has been sampled (call sample_one_video or sample_long_video first)")
    if tuple(real_vid.shape) != tuple(model.sample_out_vid.shape):
        raise ValueError("sample_against_real: real_vid %s does not match the sampled video %s"
                         % (tuple(real_vid.shape), tuple(model.sample_out_vid.shape)))
    real = _frozen_lfae(model, real_vid, model.sample_img.float())
    return {"vs_real": compare_videos(model.sample_out_vid, real, mean, domain),
            "vs_lfae": compare_videos(model.sample_out_vid, model.real_out_vid, mean, domain),
            "lfae": compare_videos(model.real_out_vid, real, mean, domain),
            "flow": compare_flows(model.sample_vid_grid, model.real_vid_grid, model.sample_vid_conf, model.real_vid_conf)}


def _sample(model, sample_img, sample_text, cond_scale, seed, total_frames, overlap, seeds=None, method="chain", blend="ramp"):
    torch.manual_seed(seed)
    model.set_sample_input(sample_img=sample_img, sample_text=sample_text)
    if total_frames:
        joint = dict(method="joint", blend=blend) if method == "joint" else {}
        model.sample_long_video(cond_scale, total_frames, overlap=overlap, **joint, **({} if seeds is None else dict(seed=seeds)))
    else:
        model.sample_one_video(cond_scale=cond_scale, **({} if seeds is None else dict(seeds=seeds)))
    return {k: getattr(model, k).clone() for k in ("sample_out_vid", "sample_vid_grid", "sample_vid_conf")}


def ab_compare(model_a, model_b, sample_img, sample_text, cond_scale=1.0, seed=0, mean=(0, 0, 0), domain="unit", total_frames=0, overlap=8,
               seeds=None, methods=("chain", "chain"), blend="ramp"):
    """Two sampling configurations on one input: B's video against A's.  Both models sample from the same source image, text and
    cond_scale directly after torch.manual_seed(seed).  Every sampler's first draw from the default generator is x_T, so both start from
    the same x_T; what follows is paired only as far as the configurations draw alike: the reference sampler (DDIM with
    eta = 1, DDPM) draws one noise tensor per step, so two such runs share their noise only step for step at equal step counts, and
    dpmpp_* draws nothing after x_T.  A model with a `noise_source` tape ignores the seed.
    seeds (one integer per video; both models built with noise="counter"): both sides sample the SAME videos - x_T, the known-frame noise of
    every window and the step noise of every step index are functions of the video's seed, so everything drawn is paired: two reference-sampler
    runs of different step counts share the noise of the step indices both have, and nothing depends on torch's generator.
    total_frames > 0: both sides sample a long video, side i by methods[i] - "chain" or "joint" (blend: the joint method's profile;
    DESIGN.md 4.17).  The two methods share x_T only where the chain's first window and the joint latent start alike: nothing else is paired.
    -> {"video": compare_videos(B, A), "flow": compare_flows(B, A)} (image-space and latent-space tables of B against A)."""
    a = _sample(model_a, sample_img, sample_text, cond_scale, seed, total_frames, overlap, seeds, methods[0], blend)
    b = _sample(model_b, sample_img, sample_text, cond_scale, seed, total_frames, overlap, seeds, methods[1], blend)
    return {"video": compare_videos(b["sample_out_vid"], a["sample_out_vid"], mean, domain),
            "flow": compare_flows(b["sample_vid_grid"], a["sample_vid_grid"], b["sample_vid_conf"], a["sample_vid_conf"])}


_SAMPLE_ATTRS = ("sample_img", "sample_text", "sample_latent", "sample_vid_grid", "sample_vid_conf", "sample_out_vid", "sample_warped_vid")


def interpolation_error(model, real_vid, ref_img, factor=2, mode="linear", mean=(0, 0, 0), domain="unit"):
    """What temporal interpolation of the latent (FlowDiffusion.decode_at) costs on real motion, on an is_train=False
    model: the frozen LFAE's pseudo-ground-truth latent of all T frames of real_vid (the grid, minus the identity under residual flow,
    and conf * 2 - 1, as the training step builds it) is thinned to frames 0, f, 2f, ... (f = factor; (T - 1) % f == 0, else ValueError),
    resampled back to the T original instants in `mode`, and both latents are decoded from ref_img.
    -> {"flow": compare_flows of the interpolated against the true maps, "video": compare_videos of the two decodes, "interp_vs_real" /
    "lfae_vs_real": compare_videos of each decode against real_vid (the second is the LFAE's own reconstruction error, the floor the
    first is read against), "held_out": (T,) bool, True where a frame was interpolated}.  Kept frames are exact copies of the latent: their
    rows of the flow table are exactly 0.  The model's sample_* attributes are left as they were."""
    f = int(factor)
    if real_vid.dim() != 5:
        raise ValueError("interpolation_error: real_vid must be (B, 3, T, H, W), got %s" % (tuple(real_vid.shape),))
    t = int(real_vid.shape[2])
    if f < 1 or f != factor or (t - 1) % f != 0:
        raise ValueError("interpolation_error: factor must be an integer >= 1 that divides T - 1 = %d, got %r" % (t - 1, factor))
    real = _frozen_lfae(model, real_vid, ref_img)
    saved = {k: getattr(model, k, None) for k in _SAMPLE_ATTRS}
    try:
        with torch.no_grad():
            grid, conf = model.real_vid_grid, model.real_vid_conf
            if model.use_residual_flow:
                b, _, _, h, w = grid.shape
                grid = grid - model.get_grid(b, t, h, w, normalize=True).to(grid.device)
            latent = torch.cat((grid, conf * 2 - 1), dim=1).contiguous()
            kept = latent[:, :, ::f].contiguous()
        model.set_sample_input(sample_img=model.ref_img, sample_text=None)
        model.decode_at(range(t), latent=latent)
        true = {k: getattr(model, k) for k in _SAMPLE_ATTRS[3:]}
        model.decode_at([j / f for j in range(t)], mode, latent=kept)
        got = {k: getattr(model, k) for k in _SAMPLE_ATTRS[3:]}
    finally:
        for k, v in saved.items():
            setattr(model, k, v)
    held_out = torch.tensor([j % f != 0 for j in range(t)], dtype=torch.bool)
    return {"flow": compare_flows(got["sample_vid_grid"], true["sample_vid_grid"], got["sample_vid_conf"], true["sample_vid_conf"]),
            "video": compare_videos(got["sample_out_vid"], true["sample_out_vid"], mean, domain),
            "interp_vs_real": compare_videos(got["sample_out_vid"], real, mean, domain),
            "lfae_vs_real": compare_videos(true["sample_out_vid"], real, mean, domain),
            "held_out": held_out}
