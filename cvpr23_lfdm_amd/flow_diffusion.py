"""Host-side mirror of the reference pipeline wrapper `FlowDiffusion`
(DM/modules/video_flow_diffusion_model.py:17-253): same constructor keywords, attributes,
setters and `sample_one_video`, so demo_*.py / test_*.py style callers can switch over.
The sampling path (a28) is fully native: LFAE encoder once per video -> hipGraph-replayed
DDIM/DDPM loop -> batched LFAE decode of all T frames.
The DM training step (a29) = frozen-LFAE pseudo ground truth batched over all frames (lfae_predictors.py) ->
diffusion loss through the native UNet forward/backward (unet_train.py, autograd.py) -> fused Adam (optim.py), with
an optional one-process-per-GPU gradient all-reduce (`enable_data_parallel`).
"""
import contextlib
import math
import os

import torch
import yaml
from torch import nn

from .diffusion import CleanRequest, GaussianDiffusion, Request
from .generator import Generator
from .params import ParamTree, bg_predictor_spec, build_tree, region_predictor_spec
from .optim import FlatAdam, GradAllReduce
from .unet import Unet3D, check_num_frames, frame_limit


class RegionPredictor(ParamTree):
    """LFAE/modules/region_predictor.py: same state-dict keys; forward = lfae_predictors.RegionPredictorExec
    (any number of frames per call)."""

    def __init__(self, num_regions, num_channels, estimate_affine=False, **params):      # (region_predictor.py:34 default)
        super().__init__()
        pca_based = params.get("pca_based", False)       # (region_predictor.py:36 default; every LFDM yaml sets pca_based: true)
        build_tree(self, region_predictor_spec(num_regions=num_regions, num_channels=num_channels, estimate_affine=estimate_affine,
                                               **dict(params, pca_based=pca_based)))
        if self.has("jacobian.weight"):                  # region_predictor.py:46-47: the regression head starts at the identity
            with torch.no_grad():
                self.get("jacobian.weight").zero_()
                self.get("jacobian.bias").copy_(torch.tensor([1, 0, 0, 1], dtype=torch.float))
        from .lfae_predictors import RegionPredictorExec
        self._exec = RegionPredictorExec(self, num_blocks=params.get("num_blocks", 5),
                                         temperature=params.get("temperature", 0.1),
                                         scale_factor=params.get("scale_factor", 0.25),
                                         pca_based=pca_based, pad=params.get("pad", 3), estimate_affine=estimate_affine)

    def forward(self, x):
        return self._exec(x)


class BGMotionPredictor(ParamTree):
    """Parameter holder for LFAE/modules/bg_motion_predictor.py."""

    def __init__(self, num_channels, **params):
        super().__init__()
        build_tree(self, bg_predictor_spec(num_channels=num_channels, **params))
        self.bg_type = params.get("bg_type", "zero")          # (bg_motion_predictor.py:20 default)
        if self.bg_type != "zero":
            from .params import BG_FC_BIAS
            with torch.no_grad():   # reference initialises fc to the identity transform (bg_motion_predictor.py:27-40)
                self.get("fc.bias").copy_(torch.tensor(BG_FC_BIAS[self.bg_type], dtype=torch.float))

        from .lfae_predictors import BGMotionPredictorExec
        self._exec = BGMotionPredictorExec(self, num_blocks=params.get("num_blocks", 5),
                                           bg_type=self.bg_type)

    def forward(self, source_image, driving_image):
        return self._exec(source_image, driving_image)


class FlowDiffusion(nn.Module):
    def __init__(self, img_size=32, num_frames=40, sampling_timesteps=250, null_cond_prob=0.1,
                 ddim_sampling_eta=1., timesteps=1000, dim_mults=(1, 2, 4, 8), lr=1e-4,
                 adam_betas=(0.9, 0.99), is_train=True, only_use_flow=True, use_residual_flow=False,
                 learn_null_cond=False, use_deconv=True, padding_mode="zeros", pretrained_pth="",
                 config_pth="", bert_path=None, *, conv_precision="fp32", sampler="reference", ema_decay=None, ema_start_step=0,
                 max_grad_norm=None, skip_nonfinite=False, long_attention=False, noise="torch", known_train=None,
                 objective="pred_noise", min_snr_gamma=None, schedule="cosine", step_grid="reference", guidance_rescale=0.0):
        """Reference signature (video_flow_diffusion_model.py:19-37) + `bert_path`: a local Hugging Face directory of
        bert-base-cased for `cond=list[str]` (the reference downloads it with torch.hub; see text.py).  LFDM_BERT_PATH in
        the environment is the default, so unchanged caller scripts pick it up.
        conv_precision (keyword only): Unet3D.conv_precision of the denoiser - "fp32" (default) or "bf16", the opt-in faster sampling mode
        whose Winograd 3x3 convolutions run on bf16 operands (sampling and the eval branch of p_losses; training stays fp32).
        sampler (keyword only): GaussianDiffusion.sampler - "reference" (default: DDIM / DDPM as the reference chooses), "dpmpp_2m"
        (DPM-Solver++(2M): second order, deterministic, meant for few steps) or "dpmpp_1"; composes with conv_precision.
        ema_decay / ema_start_step / max_grad_norm / skip_nonfinite (keyword only, all off by default; training only): FlatAdam's options -
        an exponential moving average of the denoiser's weights (`ema_weights()`, `ema_state_dict()`), global-norm gradient clipping and a
        guard that skips a step whose gradient is not finite, all decided on the device inside the optimizer step.
        long_attention (keyword only, default False): Unet3D.long_attention - up to 256 frames per window (and up to 256 pixels per frame in
        the mid block) on the streaming attention kernels, for sampling and training.
        noise (keyword only, default "torch"): GaussianDiffusion.noise - "counter" gives every sampled video a seed of its own
        (sample_one_video(seeds=...), sample_long_video(seed=...)).  Training draws stay on torch's generator.
        known_train (keyword only, default None: off): GaussianDiffusion.known_train - dict(prob=0.5, kinds=("prefix", "ends", "random"),
        max_frames=8, seed=0), random-mask training: some frames of a training video stay clean and the loss counts the others, so that
        the checkpoint can be sampled with known_level="clean" (DESIGN.md 4.12).  Not available in the functional flavour.
        objective / min_snr_gamma (keyword only, defaults "pred_noise" / None: the reference's step): GaussianDiffusion.objective - what the
        denoiser predicts, "pred_noise", "pred_x0" or "pred_v" - and the min-SNR-gamma loss weight.  A checkpoint is
        sampled with the objective it was trained with.  Not available in the functional flavour.
        schedule / step_grid / guidance_rescale (keyword only, defaults "cosine" / "reference" / 0.0: the reference's tables and launches):
        GaussianDiffusion's - "cosine_zsnr", the cosine schedule rescaled to zero terminal SNR (training and sampling; refused with
        "pred_noise"; a checkpoint is sampled on the schedule it was trained on), "trailing", the step grid that starts at the last
        timestep, and the rescale of the guided output towards the conditional output's standard deviation (sampling with cond_scale
        other than 0 and 1), after Lin et al. 2024.  In both flavours."""
        super().__init__()
        if noise not in GaussianDiffusion.NOISE_MODES:
            raise ValueError("noise must be one of %s, got %r" % (GaussianDiffusion.NOISE_MODES, noise))
        self.long_attention = bool(long_attention)
        check_num_frames(num_frames, frame_limit(self.long_attention))        # (before the checkpoint and the config are read)
        if sampler not in GaussianDiffusion.SAMPLERS:
            raise ValueError("sampler must be one of %s, got %r" % (GaussianDiffusion.SAMPLERS, sampler))
        self.use_residual_flow = use_residual_flow
        self.only_use_flow = only_use_flow
        checkpoint = torch.load(pretrained_pth, map_location="cpu") if pretrained_pth != "" else None
        with open(config_pth) as f:
            mp = yaml.safe_load(f)['model_params']
        self.lfae_config = mp                     # (video_store.lfae_fingerprint: the switches no weight records)
        self.generator = Generator(num_regions=mp['num_regions'], num_channels=mp['num_channels'],
                                   revert_axis_swap=mp['revert_axis_swap'], **mp['generator_params'])
        self.region_predictor = RegionPredictor(num_regions=mp['num_regions'], num_channels=mp['num_channels'],
                                                estimate_affine=mp['estimate_affine'],
                                                **mp['region_predictor_params'])
        self.bg_predictor = BGMotionPredictor(num_channels=mp['num_channels'], **mp['bg_predictor_params'])
        for name in ('generator', 'region_predictor', 'bg_predictor'):
            net = getattr(self, name)
            if checkpoint is not None:
                net.load_state_dict(checkpoint[name])
                net.eval()
                self.set_requires_grad(net, False)
        self.unet = Unet3D(dim=64, channels=3 + 256, out_grid_dim=2, out_conf_dim=1, dim_mults=dim_mults,
                           use_bert_text_cond=True, learn_null_cond=learn_null_cond,
                           use_final_activation=False, use_deconv=use_deconv, padding_mode=padding_mode,
                           long_attention=self.long_attention)
        self.unet.conv_precision = conv_precision
        self.diffusion = GaussianDiffusion(self.unet, image_size=img_size, num_frames=num_frames,
                                           sampling_timesteps=sampling_timesteps, timesteps=timesteps,
                                           loss_type='l2', use_dynamic_thres=True,
                                           null_cond_prob=null_cond_prob, ddim_sampling_eta=ddim_sampling_eta, sampler=sampler,
                                           long_attention=self.long_attention, noise=noise, known_train=known_train,
                                           objective=objective, min_snr_gamma=min_snr_gamma, schedule=schedule, step_grid=step_grid,
                                           guidance_rescale=guidance_rescale)
        bert_path = bert_path or os.environ.get("LFDM_BERT_PATH")
        if bert_path:
            from .text import BertTextEncoder
            self.diffusion.text_encoder = BertTextEncoder(bert_path, use_cls=self.diffusion.text_use_bert_cls)
        for attr in ('ref_img', 'ref_img_fea', 'real_vid', 'real_out_vid', 'real_warped_vid', 'real_vid_grid',
                     'real_vid_conf', 'fake_out_vid', 'fake_warped_vid', 'fake_vid_grid', 'fake_vid_conf',
                     'sample_out_vid', 'sample_warped_vid', 'sample_vid_grid', 'sample_vid_conf', 'sample_latent', 'train_latent'):
            setattr(self, attr, None)
        self.is_train = is_train
        if self.is_train:
            self.unet.train()
            self.diffusion.train()
            self.lr = lr
            self.loss = torch.tensor(0.0)
            self.rec_loss = torch.tensor(0.0)
            self.rec_warp_loss = torch.tensor(0.0)
            # a torch.optim.Optimizer (state_dict / param_groups / lr schedulers work) whose step is one fused HIP launch
            self.optimizer_diff = FlatAdam(self.diffusion.parameters(), lr=lr, betas=adam_betas, ema_decay=ema_decay,
                                           ema_start_step=ema_start_step, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        elif ema_decay is not None or max_grad_norm is not None or skip_nonfinite:
            raise ValueError("ema_decay / max_grad_norm / skip_nonfinite are options of the training optimizer: they need is_train=True")
        self._dp = None
        self.lazy_real_decode = os.environ.get("LFDM_LAZY_REAL_DECODE", "0") == "1"     # see the real_out_vid property
        self._real_decode, self._real_out_vid, self._real_warped_vid = None, None, None
        self._shard = None            # (rank, world) once data parallelism is on: set_train_input keeps this rank's videos
        self._slice = None            # (lo, hi, global batch) of the current step's shard
        # Launched by torchrun (one process per GPU) from an UNCHANGED training script: there is nobody to call
        # enable_data_parallel(), so the wrapper does it itself at the first optimize_parameters() - the process takes the
        # GPU of its LOCAL_RANK here, before the script's `.cuda()`.  LFDM_AUTO_DP=0 switches this off.
        self._auto_dp = (is_train and int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("LFDM_AUTO_DP", "1") != "0")
        if self._auto_dp and torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())

    # ------------------------------------------------------------------ sampling (a28)
    def sample_one_video(self, cond_scale, *, known_latent=None, known_mask=None, frame_times=None, interp="linear", seeds=None,
                         start_latent=None, strength=None, known_level="noised"):
        """Reference :190-216.  seeds (keyword only; noise="counter"): one integer in [0, 2^64) per video of the batch (GaussianDiffusion.sample).  Results land in sample_vid_grid (B,2,T,S,S), sample_vid_conf (B,1,T,S,S),
        sample_out_vid / sample_warped_vid (B,3,T,H,W), and the latent the diffusion returned (B,3,T,S,S; the residual flow when
        use_residual_flow) in sample_latent.  known_latent (B,3,T,S,S) in that same space + known_mask (B,T) bool (keyword only, both or
        none): GaussianDiffusion.sample's known frames.  frame_times (keyword only; default None: off) + interp: after
        sampling, decode_at(frame_times, interp) - the four result tensors then hold len(frame_times) frames.
        known_mask may also be 5-D, (B,3,T,S,S) or (B,1,T,S,S) bool: known ELEMENTS of the latent.  start_latent
        (B,3,T,S,S; e.g. `encode_video` of a real video, or an earlier sample_latent) + strength in (0, 1] (keyword only, both or none): the
        video is an edit of that latent - the schedule is entered at start_step = steps - ceil(strength * steps) on the latent noised to
        that level, so strength 1 runs every step and a small strength stays close to the start.  known_level (keyword only): "noised"
        (default) or "clean" - the known content held clean at every step, for a denoiser trained with known_train."""
        if frame_times is not None:
            frame_times = self._check_frame_times(frame_times, interp, self.diffusion.num_frames)
        dm = self.diffusion
        if (start_latent is None) != (strength is None):
            raise ValueError("sample_one_video: start_latent and strength go together (both or none)")
        start_step = 0
        if strength is not None:
            if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 < strength <= 1.0:
                raise ValueError("sample_one_video: strength must lie in (0, 1], got %r" % (strength,))
            steps = dm.sampling_timesteps if dm.is_ddim_sampling or dm.sampler != "reference" else dm.num_timesteps
            start_step = steps - int(math.ceil(strength * steps - 1e-9))        # (0.3 * 10 = 3.0000000000000004 is three steps)
        with torch.no_grad():                 # (bad known frames / seeds are refused before anything is launched)
            req = dm.check_request((self.sample_img.shape[0], dm.channels, dm.num_frames, dm.image_size, dm.image_size), known_latent, known_mask,
                                   seeds, 0, start_latent, start_step, known_level=known_level)
            img, skips, fea = self._source()
            self.sample_latent = pred = dm.sample_checked(fea, self.sample_text, cond_scale, req)
            self._decode_sample(img, skips, pred)
        if frame_times is not None:
            self.decode_at(frame_times, interp)

    def _maps(self, pred):
        """(sampling grid + occlusion channel (B,3,T,S,S), confidence (B,1,T,S,S)) of a latent (:203-210)."""
        b, nf, s = pred.shape[0], pred.shape[2], pred.shape[3]
        if self.use_residual_flow:
            grid = pred[:, :2] + self.get_grid(b, nf, s, s, normalize=True).to(pred.device)
            maps = torch.cat((grid, pred[:, 2:3]), dim=1).contiguous()
        else:
            maps = pred
        return maps, (pred[:, 2, :, :, :].unsqueeze(dim=1) + 1) * 0.5

    def _encode_source(self):
        """(img, skips) of the source image: the LFAE encoder, ONCE per (long) video."""
        img = self.sample_img.float().contiguous()
        return img, self.generator.encode(img)

    def _source(self):
        """Source image -> (img, skips, fea): the encoding and the feature map the diffusion is conditioned on (kept in sample_img_fea)."""
        img, skips = self._encode_source()
        d = 2 ** self.generator.num_down_blocks
        self.sample_img_fea = fea = self.generator.compute_fea_from_skips(skips, img.shape[0], img.shape[2] // d, img.shape[3] // d)
        return img, skips, fea

    def _decode_pieces(self, img, skips, pieces):
        """Decodes a sequence of pieces (maps (B,3,n,S,S), conf (B,1,n,S,S), n <= num_frames) - of `_maps` or ops.latent_resample_maps - into
        sample_vid_grid / sample_vid_conf / sample_out_vid / sample_warped_vid: one piece is stored as it is, several are concatenated along T."""
        cols = {"sample_vid_grid": [], "sample_vid_conf": [], "sample_out_vid": [], "sample_warped_vid": []}
        for maps, conf, n in pieces:
            s = maps.shape[3]
            out, warped = self.generator.decode_video(img, skips, maps[:, 0], maps[:, 1], maps[:, 2], n, s, s, 3 * n * s * s, s * s,
                                                      occ_scale=0.5, occ_bias=0.5)
            for col, v in zip(cols.values(), (maps[:, :2], conf, out, warped)):
                col.append(v)
        for name, col in cols.items():
            setattr(self, name, col[0] if len(col) == 1 else torch.cat(col, dim=2))

    def _decode_sample(self, img, skips, pred):
        self._decode_pieces(img, skips, [self._maps(pred) + (pred.shape[2],)])

    LONG_METHODS = ("chain", "joint")

    def joint_windows(self, total_frames, overlap):
        """The window starts of sample_long_video(method="joint") for this model's window: a list of W integers (W before window_text is
        built); refuses what the joint method refuses (ops.joint_windows)."""
        return list(self.diffusion.joint_geometry(int(total_frames), int(overlap)).starts)

    def _sample_joint_video(self, cond_scale, total_frames, overlap, blend, window_text, known_latent, known_mask, seeds, known_level):
        """sample_long_video(method="joint") behind its checks: GaussianDiffusion.sample's joint mode on ONE encoder pass -> the latent of
        total_frames frames (the global latent holds num_frames frames when total_frames is smaller: cut like the chain's)."""
        dm = self.diffusion
        with torch.no_grad():
            req, joint = dm.check_joint_request(self.sample_img.shape[0], total_frames, overlap, blend, known_latent, known_mask, seeds,
                                                known_level=known_level, window_cond=window_text)
            img, skips, fea = self._source()
            latent = dm.sample_checked(fea, None if window_text is not None else self.sample_text, cond_scale, req, joint=joint,
                                       window_cond=window_text)
        return img, skips, latent[:, :, :total_frames].contiguous()

    def sample_long_video(self, cond_scale, total_frames, overlap=8, *, method="chain", blend="ramp", window_text=None, known_latent=None,
                          known_mask=None, frame_times=None, interp="linear", seed=None, known_level="noised", start_latent=None,
                          strength=None):
        """A video of `total_frames` frames, longer than the model's window of num_frames.  method="joint" (keyword only):
        ONE latent of total_frames frames whose overlapping windows (joint_windows(total_frames, overlap)) are denoised jointly - at every
        step all windows go through the UNet as one batch and their outputs are averaged onto the global time line, weights by `blend`
        ("ramp": a window counts more towards its middle; "uniform") - so overlap frames are one set of numbers and context flows both ways.
        It takes known_latent (B,3,F,S,S) + known_mask ((B,F) bool or 5-D, as sample_one_video's) on the GLOBAL time line,
        F = max(total_frames, num_frames), and window_text: W conditions, each what sample_text is, window w uses entry w (cross-faded over
        the overlaps by the blend).  seed: one per video, counter word window = 0.  Averaging window outputs is a heuristic, not a sampler
        of a known joint distribution.  start_latent / strength are refused by both methods.
        method="chain" (default), as a chain of windows: the LFAE
        encoder runs ONCE; chunk 0 is a plain sample; chunk j > 0 is conditioned on the last `overlap` latent frames of chunk j - 1 placed at
        its frames 0 .. overlap-1 (same source image, features and text condition - only the latent is chained); the result keeps chunk 0 whole
        and frames overlap.. of every later chunk, cut to total_frames, and is decoded in pieces of at most num_frames frames.  Results as
        sample_one_video's, with T = total_frames.  frame_times / interp (keyword only): as sample_one_video's, times in
        [0, total_frames - 1].  seed (keyword only; noise="counter"): the long video's ONE seed - an integer in [0, 2^64), or one per video
        of the batch; window w draws with counter word `window` = w, so a window can be made again without the ones before it.
        known_level (keyword only): "noised" (default) or "clean" - how the overlap frames of every later window are held."""
        nf = self.diffusion.num_frames
        total_frames, overlap = int(total_frames), int(overlap)
        if overlap < 1 or overlap >= nf:
            raise ValueError("sample_long_video: overlap must lie in [1, num_frames - 1 = %d], got %d" % (nf - 1, overlap))
        if total_frames < 1:
            raise ValueError("sample_long_video: total_frames must be at least 1, got %d" % total_frames)
        if frame_times is not None:
            frame_times = self._check_frame_times(frame_times, interp, total_frames)
        dm = self.diffusion
        if known_level not in dm.KNOWN_LEVELS:
            raise ValueError("sample_long_video: known_level must be one of %s, got %r" % (dm.KNOWN_LEVELS, known_level))
        if method not in self.LONG_METHODS:
            raise ValueError("sample_long_video: method must be one of %s, got %r" % (self.LONG_METHODS, method))
        if start_latent is not None or strength is not None:
            raise ValueError("sample_long_video: start_latent / strength are not built for long videos (sample_one_video takes them)")
        if method == "chain" and (known_latent is not None or known_mask is not None):
            raise ValueError("sample_long_video: known_latent / known_mask need method='joint' (the chain conditions every window on its "
                             "predecessor's overlap frames)")
        if method == "chain" and (window_text is not None or blend != "ramp"):
            raise ValueError("sample_long_video: blend and window_text belong to method='joint'")
        with torch.no_grad():
            b, seeds = self.sample_img.shape[0], seed
            if isinstance(seed, int) and not isinstance(seed, bool):
                if b != 1:
                    raise ValueError("sample_long_video: a batch of %d videos needs a sequence of %d seeds" % (b, b))
                seeds = [seed]
            if method == "joint":
                img, skips, latent = self._sample_joint_video(cond_scale, total_frames, overlap, blend, window_text, known_latent, known_mask,
                                                              seeds, known_level)
                self.sample_latent = latent
                self._decode_pieces(img, skips, (self._maps(latent[:, :, f0:f0 + nf].contiguous()) + (min(nf, total_frames - f0),)
                                                 for f0 in range(0, total_frames, nf)))
                if frame_times is not None:
                    self.decode_at(frame_times, interp)
                return
            req = dm.check_request((b, dm.channels, nf, dm.image_size, dm.image_size), seeds=seeds)
            img, skips, fea = self._source()
            chunk = dm.sample_checked(fea, self.sample_text, cond_scale, req)
            pieces, have = [chunk], nf
            mask = torch.zeros((b, nf), dtype=torch.bool, device=chunk.device)
            mask[:, :overlap] = True
            request = CleanRequest if known_level == "clean" else Request          # how the later windows hold their overlap frames
            while have < total_frames:                                # (window w of a seeded video draws with counter word `window` = w)
                known = torch.zeros_like(chunk)
                known[:, :, :overlap] = chunk[:, :, nf - overlap:]
                window = len(pieces) if req.seeds is not None else 0
                chunk = dm.sample_checked(fea, self.sample_text, cond_scale, request(*req._replace(known=known, known_mask=mask, window=window)))
                pieces.append(chunk[:, :, overlap:])
                have += nf - overlap
            self.sample_latent = latent = torch.cat(pieces, dim=2)[:, :, :total_frames].contiguous()
            self._decode_pieces(img, skips, (self._maps(latent[:, :, f0:f0 + nf].contiguous()) + (min(nf, total_frames - f0),)
                                             for f0 in range(0, total_frames, nf)))     # in pieces of at most num_frames frames
        if frame_times is not None:
            self.decode_at(frame_times, interp)

    # ------------------------------------------------------------------ other frame times from the sampled latent
    @staticmethod
    def _check_frame_times(times, mode, frames):
        """The list of `times`, refused (ValueError / IndexError) before anything is launched when a time or the mode is bad."""
        from . import ops
        if mode not in ops.RESAMPLE_MODES:
            raise ValueError("unknown interpolation mode %r (one of %s)" % (mode, ", ".join(ops.RESAMPLE_MODES)))
        times = times.tolist() if isinstance(times, torch.Tensor) else list(times)
        ops.resample_tables(times, frames)
        return times

    def decode_at(self, times, mode="linear", *, latent=None):
        """Decodes `latent` (keyword only; default: sample_latent, what the last sample_one_video / sample_long_video left) from
        sample_img at `times`: floats in [0, T - 1] in any order, repeats allowed (retime.frame_times makes the usual lists).  An integer
        time is that sampled frame; a time between two integers is a frame whose warp field and occlusion map are interpolated between
        theirs - mode "linear", or "cubic" (Catmull-Rom; the occlusion channel is then clamped to [-1, 1]).  One launch per piece
        resamples the latent and builds the generator's maps (ops.latent_resample_maps), the batched decode runs in pieces of at most
        num_frames frames like sample_long_video's.  Results land in sample_vid_grid, sample_vid_conf, sample_out_vid and
        sample_warped_vid with len(times) frames; sample_latent is left as sampled.  decode_at(range(T)) reproduces the sampled video
        bit for bit."""
        from . import ops
        latent = self.sample_latent if latent is None else latent
        if latent is None or getattr(self, "sample_img", None) is None:
            raise RuntimeError("decode_at: nothing has been sampled yet - call sample_one_video or sample_long_video first")
        times = self._check_frame_times(times, mode, latent.shape[2])
        nf = self.diffusion.num_frames
        clamp_from = 2 if mode == "cubic" else None
        with torch.no_grad():
            img, skips = self._encode_source()
            latent = latent.to(img.device).float().contiguous()
            self._decode_pieces(img, skips, (ops.latent_resample_maps(latent, times[f0:f0 + nf], mode, residual=self.use_residual_flow,
                                                                       clamp_from=clamp_from) + (len(times[f0:f0 + nf]),)
                                             for f0 in range(0, len(times), nf)))       # in pieces of at most num_frames frames

    # ------------------------------------------------------------------ uint8 preview strips on the device
    def render_sample(self, mean=(0., 0., 0.), panels=("source", "out", "warped", "flow", "conf"), indexed=False, *, source=None):
        """The demo scripts' per-frame panel strip of the last sample_one_video / sample_long_video, rendered on the device: a uint8
        tensor (B, T, S, P*S, 3), or (B, T, S, P*S) indices into io_compat.STRIP_PALETTE (6x6x6 cube, 8x8 ordered dither) when indexed.
        panels: ordered subset of source / out / warped / flow / conf.  Image panels and conf are io_compat.sample_img(mean) / conf2fig to
        the byte; flow is the colour-coded flow of misc.flow2fig (grid2fig's line drawing is not rendered on the device).  source (keyword
        only): the (B, 3, S, S) image of the first panel, default the sample input.  Two launches (one without the flow panel)."""
        from . import ops
        if self.sample_out_vid is None:
            raise RuntimeError("render_sample: nothing has been sampled yet - call sample_one_video or sample_long_video first")
        panels = tuple(panels)
        with torch.no_grad():
            kw = {}
            if "source" in panels:
                src = self.sample_img if source is None else source
                kw["source"] = src.to(self.sample_out_vid.device).float().contiguous()
            if "out" in panels:
                kw["out_vid"] = self.sample_out_vid.contiguous()
            if "warped" in panels:
                kw["warped_vid"] = self.sample_warped_vid.contiguous()
            if "conf" in panels:
                kw["conf"] = self.sample_vid_conf.contiguous()
            if "flow" in panels:
                kw["flow_color"] = ops.flow_to_color_u8(self.sample_vid_grid)
                if "source" not in kw and len(kw) == 1:          # (a strip of the flow panel alone: the batch size comes from the source)
                    kw["source"] = self.sample_img.to(self.sample_out_vid.device).float().contiguous()
            return ops.render_strip(mean=mean, panels=panels, indexed=indexed, **kw)

    def render_sample_host(self, mean=(0., 0., 0.), panels=("source", "out", "warped", "flow", "conf"), indexed=False, *, source=None):
        """render_sample copied to the host: one asynchronous copy into a pinned buffer kept on the model (reused while the shape is
        unchanged, so the returned numpy array is overwritten by the next call of the same shape) and ONE stream synchronisation."""
        dev = self.render_sample(mean=mean, panels=panels, indexed=indexed, source=source)
        buf = getattr(self, "_render_host", None)
        if buf is None or buf.shape != dev.shape or buf.is_pinned() != dev.is_cuda:
            buf = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=dev.is_cuda)
            self._render_host = buf
        buf.copy_(dev, non_blocking=True)
        if dev.is_cuda:
            torch.cuda.current_stream(dev.device).synchronize()
        return buf.numpy()

    # ------------------------------------------------------------------ averaged weights
    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the denoiser's parameters ARE the optimizer's averaged weights (their storage is re-pointed at the `ema`
        slices, nothing is copied) and the weights epoch is bumped, so Unet3D.packed() and the captured sampling graphs rebuild:
        sample_one_video / sample_long_video sample from the average with every sampler and conv_precision.  optimizer_diff.step() raises
        inside.  The raw weights come back on exit, also when the body raises."""
        if not self.is_train:
            raise RuntimeError("ema_weights(): only a training model (is_train=True, ema_decay=...) keeps an average; for sampling alone "
                               "load ema_state_dict() into the model")
        with self.optimizer_diff.ema_weights():
            yield self

    def ema_state_dict(self):
        """A dict shaped like diffusion.state_dict() (same keys; buffers as they are) with the averaged weights in place of the raw ones,
        detached copies: what a sampling model - this framework's or the reference's demo scripts - loads with load_state_dict."""
        with self.ema_weights():
            return {k: v.detach().clone() for k, v in self.diffusion.state_dict().items()}

    def set_sample_input(self, sample_img, sample_text):
        dev = next(self.unet.parameters()).device
        self.sample_img = sample_img.to(dev)
        self.sample_text = sample_text

    # ------------------------------------------------------------------ training (a29) - next row
    def set_train_input(self, ref_img, real_vid, ref_text):
        """Reference :218-221.  Under data parallelism every rank is handed the SAME global batch (the script's DataLoader
        is seeded identically everywhere) and keeps its own contiguous slice - what nn.DataParallel's scatter does in the
        reference (DM/train_video_flow_diffusion_mhad_multiGPU.py:207,249)."""
        dev = next(self.unet.parameters()).device
        ref_img, real_vid, ref_text = self._shard_of(ref_img, real_vid, ref_text)
        self.ref_img = ref_img.to(dev)
        self.real_vid = real_vid.to(dev)
        self.ref_text = ref_text
        self.train_latent = None

    def _shard_of(self, ref_img, videos, ref_text):
        """This rank's part of a global batch (set_train_input, set_train_latent): starts data parallelism when a launcher asked for it,
        records the step's slice in `_slice` / diffusion.rank_shard and cuts the three inputs along the batch.  Without sharding the
        inputs come back as they are."""
        self._start_auto_dp()
        self._slice = None
        if self._shard is not None:
            # torch.tensor_split semantics, like nn.DataParallel's scatter: any batch size works (the reference scripts use
            # BATCH_SIZE = 5 and no drop_last); the first b % world ranks get one video more, a rank may get none
            rank, world = self._shard
            b = videos.shape[0]
            lo = rank * (b // world) + min(rank, b % world)
            hi = lo + b // world + (1 if rank < b % world else 0)
            self._slice = (lo, hi, b)
            self.diffusion.rank_shard = self._slice
            ref_img, videos = ref_img[lo:hi], videos[lo:hi]
            ref_text = ref_text[lo:hi] if isinstance(ref_text, torch.Tensor) else list(ref_text)[lo:hi]
        return ref_img, videos, ref_text

    def set_train_latent(self, ref_img, latent, ref_text):
        """The training input of a step from a STORED flow latent in place of set_train_input: latent (B, 3, T, S, S) in the
        space `encode_video` returns (video_store.DeviceLatentPrep makes it from a latent store), ref_img (B, 3, H, W).  The next
        forward() / optimize_parameters() then launches nothing of the frozen LFAE but the generator's encoder on ref_img: no region,
        background or flow predictor, no decode (see _latent_forward).  Shards like set_train_input under data parallelism."""
        dm = self.diffusion
        want = (3, dm.num_frames, dm.image_size, dm.image_size)
        if not isinstance(latent, torch.Tensor) or latent.dim() != 5 or tuple(latent.shape[1:]) != want:
            raise ValueError("set_train_latent: latent must be a (B, %d, %d, %d, %d) tensor, got %s"
                             % (want + (tuple(getattr(latent, "shape", ())),)))
        if ref_img.dim() != 4 or ref_img.shape[0] != latent.shape[0]:
            raise ValueError("set_train_latent: ref_img must be (B, 3, H, W) with the latent's batch %d, got %s"
                             % (latent.shape[0], tuple(ref_img.shape)))
        dev = next(self.unet.parameters()).device
        ref_img, latent, ref_text = self._shard_of(ref_img, latent, ref_text)
        self.ref_img = ref_img.to(dev)
        self.train_latent = latent.to(dev)
        self.real_vid = None
        self.ref_text = ref_text

    def _lfae_pass(self, real_vid, ref_img, decode):
        """The frozen LFAE on every frame of real_vid against ref_img, all B*T frames in one batched pass -> Generator.forward_frames' dict
        (optical_flow (B,2,T,S,S), occlusion_map (B,1,T,S,S), bottle_neck_feat; decode: as forward_frames' - True: prediction / deformed, False: the callable
        that makes them)."""
        b, _, nf, H, W = real_vid.shape
        with torch.no_grad():
            ref = ref_img.float().contiguous()
            frames = real_vid.float().permute(0, 2, 1, 3, 4).reshape(b * nf, -1, H, W).contiguous()
            source_region_params = self.region_predictor(ref)
            driving_region_params = self.region_predictor(frames)
            ref_rep = ref.unsqueeze(1).expand(b, nf, *ref.shape[1:]).reshape(b * nf, *ref.shape[1:])
            bg_params = self.bg_predictor(ref_rep, frames)
            return self.generator.forward_frames(ref, nf, driving_region_params, source_region_params, bg_params, decode=decode)

    def _latent_of(self, grid, conf):
        """The latent the diffusion denoises from the LFAE's sampling grid and occlusion map: grid minus identity under use_residual_flow,
        occlusion * 2 - 1."""
        if self.use_residual_flow:
            b, _, nf, h, w = grid.shape
            grid = grid - self.get_grid(b, nf, h, w, normalize=True).to(grid.device)
        return torch.cat((grid, conf * 2 - 1), dim=1)

    def encode_video(self, real_vid, ref_img):
        """The latent (B, 3, T, S, S) of a real video (B, 3, T, H, W) relative to ref_img (B, 3, H, W), in the space the diffusion denoises
        and sample_one_video(known_latent= / start_latent=) takes: the LFAE pass of the training step without the decode and without the
        diffusion.  Independent of is_train."""
        dev = next(self.unet.parameters()).device
        generated = self._lfae_pass(real_vid.to(dev), ref_img.to(dev), False)
        with torch.no_grad():
            return self._latent_of(generated["optical_flow"], generated["occlusion_map"]).contiguous()

    def _train_forward(self, real_vid, ref_img, ref_text, lazy_real=False):
        """Shared body of `forward` (reference :116-179) and of the functional *_multiGPU flavour
        (video_flow_diffusion_model_multiGPU.py:89-157): pseudo ground-truth flow / occlusion of every frame from
        the frozen LFAE (all B*T frames in one batched pass), the diffusion loss on it (native UNet forward under
        autograd), and - for the logged reconstructions - the decode of the denoised prediction.  -> dict."""
        b, _, nf, H, W = real_vid.shape
        gen = self.generator
        out = {}
        ref = ref_img.float().contiguous()
        generated = self._lfae_pass(real_vid, ref_img, not lazy_real)
        out["real_vid_grid"] = generated["optical_flow"]
        out["real_vid_conf"] = generated["occlusion_map"]
        if lazy_real:
            out["real_decode"] = generated["decode"]
        else:
            out["real_out_vid"] = generated["prediction"]
            out["real_warped_vid"] = generated["deformed"]
        out["ref_img_fea"] = generated["bottle_neck_feat"].clone().detach()
        if self.is_train:
            h, w = out["real_vid_grid"].shape[-2:]
            identity_grid = self.get_grid(b, nf, h, w, normalize=True).to(ref.device) if self.use_residual_flow else None
            grid = out["real_vid_grid"] - identity_grid if self.use_residual_flow else out["real_vid_grid"]
            res = self.diffusion(torch.cat((grid, out["real_vid_conf"] * 2 - 1), dim=1), out["ref_img_fea"], ref_text)
            if isinstance(res, tuple):
                out["loss"], out["null_cond_mask"] = res
            else:
                out["loss"] = res
            with torch.no_grad():
                pred = self.diffusion.pred_x0
                out["fake_vid_grid"] = pred[:, :2] + identity_grid if self.use_residual_flow else pred[:, :2]
                out["fake_vid_conf"] = (pred[:, 2].unsqueeze(dim=1) + 1) * 0.5
                maps = torch.cat((out["fake_vid_grid"], pred[:, 2:3]), dim=1).contiguous()
                skips = gen.encode(ref)
                fo, fw = gen.decode_video(ref, skips, maps[:, 0], maps[:, 1], maps[:, 2], nf, h, w,
                                          3 * nf * h * w, h * w, occ_scale=0.5, occ_bias=0.5)
                out["fake_out_vid"], out["fake_warped_vid"] = fo, fw
        return out

    def forward(self):
        """Reference :116-179 (inputs from set_train_input, results as attributes).  After set_train_latent: _latent_forward."""
        if self.train_latent is not None:
            return self._latent_forward()
        out = self._train_forward(self.real_vid, self.ref_img, self.ref_text, lazy_real=self.lazy_real_decode)
        for k in ("real_vid_grid", "real_vid_conf", "ref_img_fea"):
            setattr(self, k, out[k])
        if self.lazy_real_decode:
            self._real_decode, self._real_out_vid, self._real_warped_vid = out["real_decode"], None, None
        else:
            self._real_decode, self._real_out_vid, self._real_warped_vid = None, out["real_out_vid"], out["real_warped_vid"]
        if self.is_train:
            for k in ("loss", "fake_vid_grid", "fake_vid_conf", "fake_out_vid", "fake_warped_vid"):
                setattr(self, k, out[k])
            with torch.no_grad():
                self.rec_loss = (self.real_vid - self.fake_out_vid).abs().mean()
                self.rec_warp_loss = (self.real_vid - self.fake_warped_vid).abs().mean()

    # ------------------------------------------------------------------ the step from a stored latent
    def _latent_forward(self):
        """forward() after set_train_latent.  The pseudo ground truth is the stored latent, so the frozen LFAE runs only as far as the
        diffusion's condition needs it: ref_img_fea from the generator's encoder on ref_img (the bottle_neck_feat of the online pass, bit for
        bit), then self.diffusion(latent, ref_img_fea, ref_text) - the online step's call with the same draws in the same order, so
        known_train, EMA, clipping and the non-finite guard work unchanged.  real_vid_grid / real_vid_conf / fake_vid_grid / fake_vid_conf
        are set from the latent and pred_x0; the four decoded videos and the two logged numbers rec_loss / rec_warp_loss are None until
        decode_step_logs(real_vid) is asked for them.  The backward of such a step runs on `loss` alone also with only_use_flow=False: the
        two reconstruction terms are no_grad constants, so the gradient is the same."""
        gen = self.generator
        ref = self.ref_img.float().contiguous()
        with torch.no_grad():
            latent = self.train_latent.float().contiguous()
            self.ref_img_fea = gen.compute_fea(ref).clone().detach()
            maps, self.real_vid_conf = self._maps(latent)
            self.real_vid_grid = maps[:, :2]
        self._real_decode, self._real_out_vid, self._real_warped_vid = None, None, None
        self.fake_out_vid = self.fake_warped_vid = None
        self.rec_loss = self.rec_warp_loss = None
        if self.is_train:
            self.loss = self.diffusion(latent, self.ref_img_fea, self.ref_text)
            with torch.no_grad():
                maps, self.fake_vid_conf = self._maps(self.diffusion.pred_x0)
                self.fake_vid_grid = maps[:, :2]

    def decode_step_logs(self, real_vid):
        """What a latent step leaves out, on demand (the trainer asks at --save-img-freq only): real_out_vid / real_warped_vid - the LFAE
        decode of the stored latent -, fake_out_vid / fake_warped_vid - the decode of the step's pred_x0 - and rec_loss / rec_warp_loss
        against real_vid (B, 3, T, H, W; the global batch under sharded data parallelism), with the expressions forward() uses for the
        last four.  The occlusion of the real decode comes back from the latent as (ch2 + 1) * 0.5, one rounding away from the LFAE's."""
        if self.train_latent is None or self.fake_vid_grid is None:
            raise RuntimeError("decode_step_logs: no step from a stored latent has run - set_train_latent(...) and optimize_parameters() first")
        gen = self.generator
        with torch.no_grad():
            ref = self.ref_img.float().contiguous()
            real_vid = real_vid.to(ref.device)
            if self._slice is not None and real_vid.shape[0] == self._slice[2]:
                real_vid = real_vid[self._slice[0]:self._slice[1]]
            nf, h, w = (int(v) for v in self.train_latent.shape[2:])
            if ref.shape[0] == 0:          # a rank without videos this step
                vid = torch.zeros(0, 3, nf, ref.shape[-2], ref.shape[-1], device=ref.device)
                self._real_out_vid = self._real_warped_vid = self.fake_out_vid = self.fake_warped_vid = vid
                self.rec_loss, self.rec_warp_loss = torch.zeros((), device=ref.device), torch.zeros((), device=ref.device)
                return
            skips = gen.encode(ref)
            vids = []
            for grid, latent in ((self.real_vid_grid, self.train_latent.float()), (self.fake_vid_grid, self.diffusion.pred_x0)):
                maps = torch.cat((grid, latent[:, 2:3]), dim=1).contiguous()
                vids.extend(gen.decode_video(ref, skips, maps[:, 0], maps[:, 1], maps[:, 2], nf, h, w, 3 * nf * h * w, h * w,
                                             occ_scale=0.5, occ_bias=0.5))
            self._real_decode = None
            self._real_out_vid, self._real_warped_vid, self.fake_out_vid, self.fake_warped_vid = vids
            self.rec_loss = (real_vid - self.fake_out_vid).abs().mean()
            self.rec_warp_loss = (real_vid - self.fake_warped_vid).abs().mean()

    # real_out_vid / real_warped_vid (reference :139-140): the LFAE decode of the pseudo ground truth feeds no loss - the
    # training scripts only write it to their sample images every `save_img_freq` steps.  By default it is computed in
    # forward() like the reference does; with `lazy_real_decode = True` (or LFDM_LAZY_REAL_DECODE=1) the 320-frame decode
    # (a sixth of the B = 8 step) runs when one of the two attributes is first read.
    def _materialise_real(self):
        if self._real_out_vid is None and self._real_decode is not None:
            self._real_out_vid, self._real_warped_vid = self._real_decode()
            self._real_decode = None

    @property
    def real_out_vid(self):
        self._materialise_real()
        return self._real_out_vid

    @real_out_vid.setter
    def real_out_vid(self, v):
        self._real_out_vid = v

    @property
    def real_warped_vid(self):
        self._materialise_real()
        return self._real_warped_vid

    @real_warped_vid.setter
    def real_warped_vid(self, v):
        self._real_warped_vid = v

    # ------------------------------------------------------------------ progressive distillation
    def begin_distill_round(self, student_steps, teacher=None, **kw):
        """One round of progressive distillation (Salimans & Ho 2022): from here on every training step teaches `unet`, the student, to
        reach in ONE DDIM step what the frozen teacher reaches in two, on the "trailing" grid of student_steps steps.  teacher=None: a deep
        copy of the current `unet` - the student starts from the teacher's weights; keywords: GaussianDiffusion.set_distill's
        (teacher_cond_scale, teacher_guidance_rescale, distill_weight).  Sampling is set to the student's schedule: sampling_timesteps =
        student_steps, eta = 0.  forward() / optimize_parameters() are the ordinary ones - `self.diffusion(...)` is the distillation step -
        so EMA, clipping, the non-finite guard, the stored-latent step and data parallelism work unchanged; the optimizer is the caller's
        (tools/distill_dm.py resets its moments at each round, as the paper does).  end_distill() returns to ordinary training.  -> the teacher."""
        if teacher is None:
            import copy
            caches = self.unet._pk, self.unet._bufs         # (the weight pack and the scratch arenas: the copy makes its own)
            self.unet._pk, self.unet._bufs = None, {}
            try:
                teacher = copy.deepcopy(self.unet)
            finally:
                self.unet._pk, self.unet._bufs = caches
        self.diffusion.set_distill(teacher, student_steps, **kw)
        self.diffusion.sampling_timesteps = student_steps
        self.diffusion.is_ddim_sampling = student_steps < self.diffusion.num_timesteps
        self.diffusion.ddim_sampling_eta = 0.0
        return teacher

    def end_distill(self):
        self.diffusion.set_distill(None)

    def enable_data_parallel(self, bucket_bytes=64 << 20, shard_inputs=True):
        """One process per GPU (torch.distributed initialised by the launcher): average the DM gradients over the
        ranks with a bucketed RCCL all-reduce that overlaps backward.  No-op for world size 1.
        shard_inputs: every rank receives the same global batch and keeps its slice (set_train_input); the step's random
        draws (t, noise, null-condition mask) are made for the global batch and sliced, so N ranks reproduce the
        single-process step on the same batch exactly.  shard_inputs=False: the caller already feeds rank-local batches
        (tools/train_dm.py with a DistributedSampler)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            self._dp = GradAllReduce(self.optimizer_diff, bucket_bytes=bucket_bytes)
            self._dp.sync_replicas()          # rank 0's parameters + Adam moments -> all ranks, once
            if shard_inputs:
                self._shard = (dist.get_rank(), dist.get_world_size())
                self.diffusion.rank_shard = self._shard
        return self

    def _start_auto_dp(self):
        if not self._auto_dp or self._dp is not None:
            return
        import torch.distributed as dist
        if not dist.is_initialized():
            backend = os.environ.get("LFDM_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")     # "nccl" = RCCL
            dist.init_process_group(backend)
        self._auto_dp = False
        self.enable_data_parallel()

    def optimize_parameters(self):
        """:181-188.  Under sharded data parallelism the rank's loss is the mean over ITS videos: it is weighted by
        shard_size * world / global_batch before backward, so that the all-reduced sum times 1/world (folded into the Adam
        kernel) is the gradient of the mean over the global batch for any split; a rank without videos this step skips the
        model, advances the random generator like everybody else and contributes zero gradients."""
        weight, empty = 1.0, False
        latent_step = self.train_latent is not None          # (after set_train_latent: DESIGN.md 4.13)
        if self._dp is not None and getattr(self, "_slice", None) is not None:
            lo, hi, total = self._slice
            weight, empty = (hi - lo) * self._shard[1] / float(total), hi == lo
        if empty:
            dev = next(self.unet.parameters()).device
            s = self.diffusion.image_size
            # (forward() calls self.diffusion(x, fea, text) without focus arguments: prob_focus_present = 0, no focus-mask draw to replay)
            self.diffusion.skip_step_draws(self._slice[2], (3, self.diffusion.num_frames, s, s), dev, prob_focus_present=0.)
            self.unet.null_cond_mask = torch.zeros(0, dtype=torch.bool, device=dev)
            self.loss = torch.zeros((), device=dev)
            self.rec_loss, self.rec_warp_loss = torch.zeros((), device=dev), torch.zeros((), device=dev)
            # what the training scripts read after a step (sample images, logs): zero-video tensors of the right rank, so an empty
            # rank's first step does not meet attributes that only forward() would have created
            nf, hw = self.diffusion.num_frames, self.real_vid.shape[-1] if getattr(self, "real_vid", None) is not None else 4 * s
            vid = torch.zeros(0, 3, nf, hw, hw, device=dev)
            self.real_vid_grid = self.fake_vid_grid = torch.zeros(0, 2, nf, s, s, device=dev)
            self.real_vid_conf = self.fake_vid_conf = torch.zeros(0, 1, nf, s, s, device=dev)
            self.ref_img_fea = torch.zeros(0, 256, s, s, device=dev)
            if latent_step:          # as _latent_forward leaves them: decode_step_logs makes the zero-video tensors when asked
                vid = self.rec_loss = self.rec_warp_loss = None
            self.fake_out_vid = self.fake_warped_vid = vid
            self._real_decode, self._real_out_vid, self._real_warped_vid = None, vid, vid
            self.optimizer_diff.zero_grad()
            self._dp.prepare()
            self._dp.finish()
            self.optimizer_diff.step()
            return
        self.forward()
        self.optimizer_diff.zero_grad()
        if self._dp is not None:
            self._dp.prepare()
        # (a latent step has no reconstruction terms: they are no_grad constants, the gradient is that of `loss` either way)
        total_loss = self.loss if self.only_use_flow or latent_step else self.loss + self.rec_loss + self.rec_warp_loss
        (total_loss * weight if weight != 1.0 else total_loss).backward()
        if self._dp is not None:
            self._dp.finish()
        self.optimizer_diff.step()

    # ------------------------------------------------------------------ misc (reference :227-253)
    def print_learning_rate(self):
        lr = self.optimizer_diff.param_groups[0]['lr']
        assert lr > 0
        print('lr= %.7f' % lr)

    def get_grid(self, b, nf, H, W, normalize=True):
        """linspace(-1,1) identity grid in (x, y) order, (B, 2, nf, H, W) (:232-240)."""
        ys = torch.linspace(-1, 1, H) if normalize else torch.arange(0, H).float()
        xs = torch.linspace(-1, 1, W) if normalize else torch.arange(0, W).float()
        gy, gx = ys.view(H, 1).expand(H, W), xs.view(1, W).expand(H, W)
        grid = torch.stack((gx, gy), dim=0).float()
        return grid.view(1, 2, 1, H, W).repeat(b, 1, nf, 1, 1)

    def set_requires_grad(self, nets, requires_grad=False):
        if not isinstance(nets, list):
            nets = [nets]
        for net in nets:
            if net is not None:
                for p in net.parameters():
                    p.requires_grad = requires_grad


class FlowDiffusionFunctional(FlowDiffusion):
    """The *_multiGPU.py flavour of the wrapper (DM/modules/video_flow_diffusion_model_multiGPU.py): functional
    `forward(real_vid, ref_img, ref_text) -> dict` with an un-reduced `loss` and `null_cond_mask`, functional
    `sample_one_video(sample_img, sample_text, cond_scale) -> dict`, optimizer owned by the training script
    (DM/train_video_flow_diffusion_mhad_multiGPU.py:182,249-299,357).  Data parallelism is one process per GPU here
    (wrap the script's optimizer step with `GradAllReduce`, or use `FlowDiffusion.enable_data_parallel`)."""

    def __init__(self, *args, **kwargs):
        kwargs.pop("lr", None)
        super().__init__(*args, **kwargs)
        self.diffusion.per_element_loss = True

    def set_train_latent(self, *args, **kwargs):
        raise NotImplementedError("set_train_latent: the step from a stored latent is FlowDiffusion's; the functional flavour takes its "
                                  "inputs through forward(real_vid, ref_img, ref_text)")

    def forward(self, real_vid, ref_img, ref_text):
        out = self._train_forward(real_vid, ref_img, ref_text)
        if self.is_train:
            with torch.no_grad():
                out["rec_loss"] = (real_vid - out["fake_out_vid"]).abs()
                out["rec_warp_loss"] = (real_vid - out["fake_warped_vid"]).abs()
        out.pop("ref_img_fea", None)
        return out

    def sample_one_video(self, sample_img, sample_text, cond_scale, *, known_latent=None, known_mask=None, frame_times=None, interp="linear",
                         seeds=None, start_latent=None, strength=None, known_level="noised"):
        self.set_sample_input(sample_img=sample_img, sample_text=sample_text)
        FlowDiffusion.sample_one_video(self, cond_scale, known_latent=known_latent, known_mask=known_mask, frame_times=frame_times,
                                       interp=interp, seeds=seeds, start_latent=start_latent, strength=strength, known_level=known_level)
        return {k: getattr(self, k) for k in ("sample_vid_grid", "sample_vid_conf", "sample_out_vid", "sample_warped_vid", "sample_latent")}
