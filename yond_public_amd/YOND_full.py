"""Full-frame evaluation drivers: the entry points README.md:38-47 names (YOND_any / YOND_ELD / YOND_LRID / YOND_DND) but the
reference does not ship.  They are modelled on YOND_SIDD.py with the full-frame runfiles it does ship
(runfiles/YOND/{ANY,ELD,LRID}_simple+full_pre_grumix.yml: `full_dn: True`, `iter`, clip False, `ratio_list`, `cam_list`):

    python YOND_any.py  -f runfiles/YOND/ANY_simple+full_pre_grumix.yml  -m eval
    python YOND_ELD.py  -f runfiles/YOND/ELD_simple+full_pre_grumix.yml  -m eval
    python YOND_LRID.py -f runfiles/YOND/LRID_simple+full_pre_grumix.yml -m eval
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 YOND_ELD.py -f ... -m eval
    python YOND_any.py  -f runfiles/YOND/ANY_simple+full_pre_grumix.yml  -m eval --save dn16     # + <result_dir>/<method_name>/<name>.{npy,json}

Per (camera,) ratio of the runfile's list the dataset is switched with `change_eval_ratio` (data_process/yond_datasets.py:912,
1033), every frame goes through `IterDenoise` as ONE whole-frame forward per round (YOND_SIDD.py:387-389, 456-458) with
p = {wp, bl, ratio, scale = (wp - bl) / ratio} (:503-505), and PSNR / SSIM of the whole frame are accumulated per ratio.
Frames are sharded one per GPU process (frame k -> rank k mod world); the metric sums are reduced with ONE all-reduce per
ratio.  Datasets are `.npy`-converted trees (yond_public_amd/data.py: rawpy is not in this image); without any data the
driver runs on seeded synthetic low-light frames of the runfile's H x W so that the control flow can be exercised and timed.

The two ends of a frame's trip are kernels (yond_public_amd/rawio.py): the datasets hand the raw DN over as loaded (uint16 or
float32), the loader threads upload them in that dtype and normalise on the device (`--host-ingest`: the NumPy expression on the
host, as before); `--save dn16 | f32` writes every item's last round through a FrameWriter, as uint16 DN at the level of the frame
the metrics were computed on (the digital gain kept) or as float32 in the [0, 1] scale, each with a JSON sidecar.

`--synth-noise K,SIGMA` closes the loop for the blind estimator on a user's own frames: every item's clean frame (hr if present,
else lr) is the ground truth, the noisy frame is made from it on the GPU (yond_public_amd/pgnoise.py: Poisson-Gaussian with system
gain K and read noise SIGMA in DN of wp - bl, exposed at 1 / ratio, not clipped, noise key crc32(name)), and beside PSNR / SSIM the
log and `metrics[name]` carry the true level and the estimator's relative error per round -- both in the estimate's own units, DN of
the frame the pipeline is handed (digital gain included: ratio * K, ratio * SIGMA).  Without data the synthetic frames then
hand out the clean frame only: no host Poisson draw in the loader threads.

`--camera-noise SPEC` does the same with the low-light camera model (yond_public_amd/camnoise.py: Poisson or Gaussian shot noise,
Tukey-lambda or Gaussian read noise, row noise, quantisation, dark bias; SPEC in DN at capture, e.g.
code=pgrq,K=0.22,sigTL=0.76,sigGs=1.26,sigR=0.23,lam=-0.026): how far do the Poisson-Gaussian line fit and the denoiser drift under
banding and heavy tails.  The truth it reports is the Poisson-Gaussian level with the model's variance (camnoise.effective_pg:
ratio * K, ratio * sigma_eff); the dark bias is a mean offset, logged and kept in `metrics[name]['bias']`, not part of the error.
The two flags exclude each other.

`--illum-corr frame | cfa` (runfile: pipeline.illum_corr) adds the ELD protocol's illuminance correction to the metrics
(yond_public_amd/illum.py; the reference's IlluminanceCorrect, data_process/__init__.py:139-171): a frame exposed at 1 / ratio and
multiplied back carries its black-level error as a global brightness error, which one least-squares gain against the unsaturated
ground truth removes before PSNR / SSIM.  The plain metrics stay where they are; `psnr_ic`, `ssim_ic`, `illum_gain` and the
`*_ic_*` means are reported beside them.  Saved frames stay uncorrected (the correction needs the ground truth); their sidecar
carries the gain.

`--noise-kld est | K,SIGMA | cam:SPEC` (runfile: pipeline.noise_kld, noise_kld_range, noise_kld_bands) reports how well a noise model
explains each paired frame's noise (yond_public_amd/noisekld.py; the reference's cal_kld, utils/sidd_utils.py:280-304): the KL
divergence between the histogram of lr - hr and the histogram of residuals the model draws on hr -- `est`: the last round's blind
estimate, already in the units of the frame the pipeline is handed (exposure 1); `K,SIGMA`: a Poisson-Gaussian level in DN at capture,
the ratio applied as --synth-noise applies it; `cam:SPEC`: the camera model of --camera-noise.  `metrics[name]` gains kld, kld_cfa (the
four CFA positions), kld_bands (`--kld-bands N` intensity bands of hr) and kld_floor, the model against itself under a second noise key:
the sampling noise any value has to clear.  The noise keys are crc32(name + '/kld0') and crc32(name + '/kld1').

`--bad-pixels FILE.npy | auto | auto:T` (runfile: pipeline.bad_pixels) takes hot and dead pixels out of every frame before it is estimated
and denoised (yond_public_amd/bpc.py): FILE.npy is the camera's bad-point list, int [n][2] of (row, col), repaired as the reference's
repair_bad_pixels does (utils/isp_ops.py:152-160: the 3x3 median of the point's own CFA plane); `auto` has no list -- one blind estimate
of the frame (SimpleNLF, the runfile's k) gives the noise model, and a pixel that stands out from all eight same-colour neighbours by T
standard deviations (default 6) is repaired in one pass; the pipeline then estimates again on the repaired frame.  The rule is this
project's extension; two touching same-colour defects hide each other (a list handles clusters).  `metrics[name]['bad_pixels']` is
{'hot', 'cold'}; the --save sidecar carries it and, in auto mode, up to 4096 coordinates.
`--synth-defects N[,LEVEL]` (with --synth-noise / --camera-noise) sets N isolated stuck pixels in the noisy frame, keyed by
crc32(name + '/defects'); the ground truth stays clean, and `metrics[name]['defects']` is {'n', 'found', 'false'} against that truth.

`--row-denoise [SPEC]` (runfile: pipeline.row_denoise) takes row noise (banding) out of every frame before it is estimated and denoised
(yond_public_amd/rownoise.py, the reference's row_denoise, utils/isp_algos.py:319-334), after the noise synthesis, --synth-defects and
--bad-pixels: a stuck pixel at the white level shifts its row's mean, so defects go first.  SPEC is empty or `on`, or
sc=10,ss=auto,d=25,per=row|plane: sc is sigma_color in DN at capture (the frame handed on is (DN - bl) / (wp - bl) * ratio, so the
filter gets sc * ratio / (wp - bl)), ss=auto is 1 + ISO / 200 from the item's ISO (1600 for an item without one, said once in the log),
per=plane removes one offset per row of a CFA plane.  `metrics[name]['row_noise']` is {'sigma', 'max'}, the RMS and the largest
magnitude of the removed offsets in DN at capture; the --save sidecar carries the same.  The ground truth is untouched.  The method
assumes smooth row means: on a scene, content leaks into the offsets (rownoise.py names the figures).
"""
import os
import time
import zlib

import numpy as np
import torch
import yaml

from . import archs as _archs
from . import bpc as BP
from . import camnoise as CN
from . import data as _data
from . import distributed as D
from . import illum as IL
from . import noisekld as NK
from . import pgnoise as PG
from . import pipeline as P
from . import rownoise as RN
from . import synthetic as S
from .YOND_SIDD import YONDParser, load_estimators, log

STREAM_EVAL = True                 # eval(): frames through pipeline.denoise_stream (False: IterDenoise one frame at a time, synchronised after every frame)


class SyntheticFrames:
    """Stand-in when the runfile's root_dir holds no frames: low-light Poisson-Gaussian frames of the runfile's size.
    clean_only (the driver's --synth-noise): the clean frame alone, the driver makes the noise on the device."""

    def __init__(self, n, H, W, K=2.0, sigma=8.0, clean_only=False):
        self.n, self.H, self.W, self.K, self.sigma, self.ratio, self.clean_only = n, H, W, K, sigma, 1, bool(clean_only)

    def __len__(self):
        return self.n

    def change_eval_ratio(self, *a, **kw):
        self.ratio = kw.get('ratio', a[-1] if a else 1)

    def __getitem__(self, k):
        rng = np.random.default_rng(4000 + k)
        clean = (S.synth_clean(self.H, self.W) * (0.6 / self.ratio)).astype(np.float32)       # exposure 1 / ratio ...
        if self.clean_only:
            return {'hr': (clean * self.ratio).astype(np.float32), 'name': f'synthetic_{k:03d}_x{self.ratio:02d}', 'ratio': self.ratio,
                    'cfa': 'rggb', 'meta': None}
        noisy = (rng.poisson(clean * 959.0 / self.K) * self.K + rng.normal(0.0, self.sigma, clean.shape)) / 959.0
        return {'lr': (noisy * self.ratio).astype(np.float32), 'hr': (clean * self.ratio).astype(np.float32),   # ... digital gain = ratio
                'name': f'synthetic_{k:03d}_x{self.ratio:02d}', 'ratio': self.ratio, 'cfa': 'rggb', 'meta': None}


class YOND_Full:
    on_result = None               # callable(name, res): called with every item's result right before it is accounted, on the consumer stream
    on_input = None                # callable(name, lr): called with every item's frame as it is handed to the pipeline (after noise, defects, repair and row denoising)

    def __init__(self, args=None):
        self.parser = YONDParser().parse(args)
        with open(self.parser.runfile, 'r', encoding='utf-8') as f:
            self.args = yaml.load(f.read(), Loader=yaml.FullLoader)
        self.mode = self.args['mode'] if self.parser.mode is None else self.parser.mode
        self.rank, self.local_rank, self.world = D.init()
        if not torch.cuda.is_available():
            raise SystemExit("the full-frame drivers need an MI355X: the HIP path has no CPU fallback")
        self.device = torch.device('cuda', self.local_rank)
        torch.cuda.set_device(self.device)
        self.synth_noise = getattr(self.parser, 'synth_noise', None)    # (K, sigma) in DN, or None
        self.camera_noise = getattr(self.parser, 'camera_noise', None)  # the --camera-noise spec (camnoise.camera_noise_arg), or None
        if self.synth_noise is not None and self.camera_noise is not None:
            raise SystemExit("--synth-noise and --camera-noise exclude each other: one noise model makes the frames (--camera-noise code=p,K=..,sigGs=.. "
                             "is --synth-noise K,SIGMA)")
        # the Poisson-Gaussian level in DN at capture that the estimator is measured against, whichever flag makes the noise
        self.true_level = self.synth_noise
        if self.camera_noise is not None:
            self.true_level = CN.effective_pg(self.camera_noise, self.camera_noise['code'], self.camera_noise['mfm'])
        self.arch, self.pipe = self.args['arch'], dict(self.args['pipeline'])
        if self.pipe.get('bias_corr') == 'none':
            self.pipe['bias_corr'] = None
        self.pipe.setdefault('k', 29)                                   # (the ANY runfile leaves k to the driver's default)
        if getattr(self.parser, 'fit', None) is not None:               # --fit overrides the runfile's pipeline.est_fit
            self.pipe['est_fit'] = self.parser.fit
        self.fit = P.est_fit_of(self.pipe)                              # 'ransac': frames take IterDenoise one at a time (stream_applies)
        if getattr(self.parser, 'illum_corr', None) is not None:        # --illum-corr overrides the runfile's pipeline.illum_corr
            self.pipe['illum_corr'] = self.parser.illum_corr
        self.illum_corr = IL.illum_corr_of(self.pipe)                   # 'off' | 'frame' | 'cfa': the metrics' illuminance correction
        self.pipe.pop('illum_corr', None)                               # (the drivers' own key: nothing of the pipeline reads it)
        # --noise-kld / --kld-range / --kld-bands override the runfile's pipeline.noise_kld / noise_kld_range / noise_kld_bands
        self.noise_kld, self.kld_range, self.kld_bands = NK.noise_kld_of(self.pipe, self.parser)
        for key in ('noise_kld', 'noise_kld_range', 'noise_kld_bands'):
            self.pipe.pop(key, None)
        # --bad-pixels overrides the runfile's pipeline.bad_pixels: None | ('list', path) | ('auto', t)
        self.bad_pixels = BP.bad_pixels_of(self.pipe, self.parser)
        self.pipe.pop('bad_pixels', None)
        self.synth_defects = getattr(self.parser, 'synth_defects', None)    # (n, level or None), or None
        if self.synth_defects is not None and self.true_level is None:
            raise SystemExit("--synth-defects sets stuck pixels in the noisy frame the driver makes: it needs --synth-noise or --camera-noise")
        self.bad_points = None                                              # the list of --bad-pixels FILE.npy: (host int32 [n][2], device copy)
        if self.bad_pixels is not None and self.bad_pixels[0] == 'list':
            pts = BP.load_points(self.bad_pixels[1])
            self.bad_points = (pts, torch.from_numpy(pts).to(self.device))  # uploaded once per run
        # --row-denoise overrides the runfile's pipeline.row_denoise: None | {'sc', 'ss', 'd', 'per'}
        self.row_denoise = RN.row_denoise_of(self.pipe, self.parser)
        self.pipe.pop('row_denoise', None)
        if not self.pipe.get('full_dn', False):
            raise SystemExit(f"{self.parser.runfile}: the full-frame drivers run runfiles with `full_dn: True` (YOND_SIDD.py handles the block layout)")
        self.model_name, self.method_name = self.args['model_name'], self.args['method_name']
        os.makedirs('./logs', exist_ok=True)
        self.logfile = f'./logs/log_{self.method_name}.log' if self.rank == 0 else None
        self.net = getattr(_archs, self.arch['name'])(self.arch)
        for suffix in ('_best_model.pth', '_last_model.pth', '.pth'):                         # YOND_SIDD.py:178-182
            model_path = f"{self.args['fast_ckpt']}/{self.model_name}{suffix}"
            if os.path.exists(model_path):
                self.net.load_state_dict(torch.load(model_path, map_location='cpu'))
                break
        else:
            model_path = None
            self.net.load_state_dict(S.denoising_state_dict(self.net, 0))
        self.net = self.net.to(self.device).eval()
        self.est_args, self.est_net = load_estimators(self.args, self.device, self.logfile if self.rank == 0 else None)
        self.biaslut = P.BiasLUT() if os.path.exists('checkpoints/bias_lut_2d.npy') else None
        if self.rank == 0:
            log(f'Method Name:\t{self.method_name}', self.logfile, notime=True)
            log(f'Checkpoint:\t{model_path or "none found -> synthetic denoising weights (timing / parity only)"}', self.logfile, notime=True)
            log(f"Let's use {self.world} GPUs (one process each, image-parallel)!", self.logfile, notime=True)
        self.change_eval_dst('test' if 'test' in self.mode else 'eval')

    def change_eval_dst(self, mode='eval'):
        self.dst = dict(self.args[f'dst_{mode}'])
        cls = self.dst.get('dataset', 'Any_Dataset')
        table = {'ELD_Full_Dataset': _data.ELD_Full_Dataset, 'LRID_Dataset': _data.LRID_Dataset, 'Any_Dataset': _data.Any_Dataset}
        self.dst_eval = None
        if cls in table and os.path.isdir(str(self.dst.get('root_dir', ''))):
            ds = table[cls](self.dst)
            if len(ds) or cls != 'Any_Dataset':
                self.dst_eval = ds
        if self.dst_eval is None or (len(self.dst_eval) == 0 and cls == 'Any_Dataset'):
            self.dst_eval = SyntheticFrames(self.parser.synthetic, int(self.dst.get('H', 3472)), int(self.dst.get('W', 4624)),
                                            clean_only=self.true_level is not None)

    def synthesise(self, data, wp, bl):
        """--synth-noise / --camera-noise: the item's clean frame becomes its ground truth and a noisy frame made from it on the current
        stream its input (one yond_pg_noise_f32 or yond_camera_noise_f32 launch; the same name gives the same noise)."""
        clean = data['hr'] if data.get('hr') is not None else data['lr']
        if not isinstance(clean, torch.Tensor):
            clean = torch.from_numpy(np.ascontiguousarray(clean, np.float32))
        clean = clean.to(self.device, torch.float32).contiguous()
        data['hr'] = clean
        key = zlib.crc32(str(data['name']).encode())
        if self.camera_noise is not None:
            spec = self.camera_noise
            data['lr'] = CN.add_camera_noise(clean, dict(spec, wp=wp, bl=bl), spec['code'], wp - bl, key, [0], layout=CN.LAYOUT_BAYER,
                                             ratio=float(data.get('ratio', 1)), mfm=spec['mfm'], clip=spec['clip'])
            return data
        K, sigma = self.synth_noise
        data['lr'] = PG.add_pg_noise(clean, K, sigma, wp - bl, key, [0], exposure=1.0 / float(data.get('ratio', 1)))
        return data

    def repair(self, data, wp=None, bl=None):
        """--synth-defects, then --bad-pixels, then --row-denoise, on the item's input frame.  data['defects_truth']: the injected sites;
        data['bad_pixels']: {'hot', 'cold'} (list mode: listed points above / below their median) and, in auto mode, 'points', 'overflow',
        'model'; data['row_noise']: {'sigma', 'max'} of the removed offsets in DN at capture."""
        lr = data['lr']
        if not isinstance(lr, torch.Tensor):
            lr = torch.from_numpy(np.ascontiguousarray(lr, np.float32))
        lr = lr.to(self.device, torch.float32).contiguous()
        if self.synth_defects is not None:
            n, level = self.synth_defects
            if n > lr.numel() // 2000 and not getattr(self, '_defects_noted', False):
                self._defects_noted = True
                log(f"[rank {self.rank}] warning: --synth-defects {n} on a {lr.shape[0]} x {lr.shape[1]} frame is a density above 5e-4, far beyond a real "
                    "sensor's: the blind noise estimates of so defective a frame may be no noise model, and the run can stop in the bias LUT "
                    "(YOND_EINVAL), with or without --bad-pixels", self.logfile)
            lr, data['defects_truth'] = BP.inject_defects(lr, n, zlib.crc32((str(data['name']) + '/defects').encode()), level,
                                                          ratio=float(data.get('ratio', 1)))
        if self.bad_pixels is not None and self.bad_pixels[0] == 'list':
            pts, d_pts = self.bad_points
            BP.check_points(pts, tuple(lr.shape))                # every frame's shape against the list
            fixed = BP.repair_bad_pixels(lr, d_pts)
            if len(pts):
                idx = d_pts.long()
                before, after = lr[idx[:, 0], idx[:, 1]], fixed[idx[:, 0], idx[:, 1]]
                hot, cold = (int(v) for v in torch.stack([(before > after).sum(), (before < after).sum()]).cpu())
            else:
                hot = cold = 0
            data['bad_pixels'] = {'hot': hot, 'cold': cold, 'points': pts, 'overflow': False}
            lr = fixed
        elif self.bad_pixels is not None:
            t = self.bad_pixels[1]
            beta1, beta2 = (float(v) for v in P.SimpleNLF(lr, k=self.pipe.get('k', 29), setting={'mode': 'self'}))
            beta2 = max(beta2, 0.0) if np.isfinite(beta2) else beta2
            if not (np.isfinite(beta1) and np.isfinite(beta2)) or beta1 < 0 or (beta1 == 0 and beta2 == 0):
                log(f"[rank {self.rank}] warning: {data['name']}: the blind estimate beta1={beta1:g}, beta2={beta2:g} is no noise model: "
                    "--bad-pixels auto skipped for this frame", self.logfile)
                data['bad_pixels'] = {'hot': 0, 'cold': 0, 'points': np.zeros((0, 2), np.int32), 'overflow': False, 'model': None}
            else:
                lr, info = BP.detect_and_repair(lr, beta1, beta2, t, coords=BP.MAX_SAVED_POINTS)
                data['bad_pixels'] = dict(info, model=(beta1, beta2, t))
        if self.row_denoise is not None:
            spec = self.row_denoise
            iso = data.get('ISO')
            if iso is None and spec['ss'] == 'auto' and not getattr(self, '_iso_noted', False):
                self._iso_noted = True
                log(f"[rank {self.rank}] --row-denoise ss=auto: {data['name']} carries no ISO: ISO {RN.DEFAULT_ISO} assumed for such items "
                    f"(sigma_space = {1 + RN.DEFAULT_ISO / 200:g})", self.logfile)
            sc, ss, dn_per_unit = RN.frame_units(spec, data.get('ratio', 1), wp, bl, iso)
            lr, offsets = RN.row_denoise(lr, sigma_color=sc, sigma_space=ss, d=spec['d'], per=spec['per'], return_offsets=True)
            data['row_noise'] = RN.offsets_report(offsets, dn_per_unit)
        data['lr'] = lr
        return data

    def model_kld(self, data, res, wp, bl):
        """--noise-kld: {'kld', 'kld_cfa', 'kld_bands', 'kld_floor'} of one paired item -- the real residual lr - hr against the model's
        residual on hr, and the model against itself under a second key.  One histogram pass per frame splits bands and CFA positions;
        the marginal is their integer sum.  The Poisson-Gaussian models take the fused launch (no noisy frame is stored), the camera
        model yond_camera_noise_f32 and then the histogram."""
        dev = lambda t: (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, np.float32))).to(self.device, torch.float32).contiguous()
        clean, noisy = dev(data['hr']), dev(data['lr'])
        edges = NK.kld_edges(self.kld_range)
        bands = NK.band_thresholds(self.kld_bands)
        keys = [zlib.crc32((str(data['name']) + tag).encode()) for tag in ('/kld0', '/kld1')]
        ratio = float(data.get('ratio', 1))
        kind = self.noise_kld[0]
        if kind == 'cam':
            spec = self.noise_kld[1]
            draw = lambda key: NK.residual_hist(CN.add_camera_noise(clean, dict(spec, wp=wp, bl=bl), spec['code'], wp - bl, key, [0], layout=CN.LAYOUT_BAYER,
                                                                    ratio=ratio, mfm=spec['mfm'], clip=spec['clip']), clean, edges, bands)
        else:
            # est: (K, sigma) of the last round, DN of the frame the pipeline was handed; K,SIGMA: DN at capture, exposed at 1 / ratio
            K, sigma, exposure = (float(res['params'][-1][0]), float(res['params'][-1][1]), 1.0) if kind == 'est' else \
                (self.noise_kld[1], self.noise_kld[2], 1.0 / ratio)
            if not (np.isfinite(K) and np.isfinite(sigma)):
                return None                                      # (an estimate that is no number models nothing)
            draw = lambda key: NK.pg_model_hist(clean, K, max(sigma, 0.0), wp - bl, key, edges, bands, exposure=exposure)
        real, q0, q1 = NK.residual_hist(noisy, clean, edges, bands), draw(keys[0]), draw(keys[1])
        out = NK.kld_report(real, q0, clean.numel())
        out['kld_floor'] = NK.kld_report(q1, q0, clean.numel())['kld']
        return out

    def IterDenoise(self, data, params):
        return P.IterDenoise(data['lr'], self.net, self.arch, self.pipe, p=params['p'], device=self.device,
                             log=(lambda s: log(s, self.logfile)) if self.parser.verbose else None, biaslut=self.biaslut,
                             est={'est_net': self.est_net.get('est_net'), 'est_args': self.est_args})

    def _sweeps(self):
        """(label, switch) per evaluated subset: ratio_list x cam_list as the runfile gives them."""
        ratios = self.dst.get('ratio_list', [self.dst.get('ratio', 1)])
        cams = self.dst.get('cam_list', [None])
        for cam in cams:
            for ratio in ratios:
                if cam is None:
                    yield f'x{ratio}', (lambda r=ratio: self.dst_eval.change_eval_ratio(ratio=r))
                else:
                    yield f'{cam} x{ratio}', (lambda c=cam, r=ratio: self.dst_eval.change_eval_ratio(c, ratio=r)
                                              if not isinstance(self.dst_eval, SyntheticFrames) else self.dst_eval.change_eval_ratio(ratio=r))

    def eval(self, epoch=-1):
        save = getattr(self.parser, 'save', 'none')
        writer = None
        if save != 'none':
            from .rawio import FrameWriter
            self.save_dir = os.path.join(str(self.args.get('result_dir', './images')), f'{self.method_name}')
            writer = FrameWriter(self.save_dir, save)        # (under torchrun every rank writes its own frames)
        try:
            return self._eval(writer)
        finally:
            if writer is not None:
                writer.close()

    def _eval(self, writer):
        n_it = self.pipe['max_iter'] + 1 if self.pipe.get('iter') == 'iter' else 1
        results = {}
        self.metrics = {}
        for label, switch in self._sweeps():
            switch()
            ds = self.dst_eval
            wp, bl = float(getattr(ds, 'wp', self.dst.get('wp', 1023))), float(getattr(ds, 'bl', self.dst.get('bl', 64)))
            sums = D.MetricSums(n_it)
            ic_sums = D.MetricSums(n_it) if self.illum_corr != 'off' else None       # the illuminance-corrected meters
            ic_gain_sums = [0.0] * (2 * n_it)                    # per round [sum of the frames' total gains, frames that had one]
            rel_sums = [0.0] * (4 * n_it)                        # --synth-noise: per round [sum, frames] of K's and of sigma's relative error
            kld_sums = [0.0] * 3                                 # --noise-kld: [sum of KLD, sum of the floors, frames]
            device_ingest = hasattr(ds, 'raw_items') and not getattr(self.parser, 'host_ingest', False)
            if hasattr(ds, 'raw_items'):
                ds.raw_items = device_ingest                 # raw DN in the items, normalised on the device by the loader threads
            mine = D.shard_dataset(ds, self.rank, self.world)
            torch.cuda.synchronize()
            t0, t_path, npix = time.perf_counter(), 0.0, 0
            from .data import Prefetcher                     # loader threads read / convert / upload the frames ahead of the GPU
            loader = Prefetcher(ds, mine, self.device, upload=('lr', 'hr'), depth=getattr(self.parser, 'prefetch', 4), workers=getattr(self.parser, 'loaders', 4),
                                ingest=device_ingest)

            def params_of(data):
                p = dict(self.pipe)
                p.update({'wp': wp, 'bl': bl, 'ratio': data.get('ratio', 1), 'gain': 1, 'sigma': 0})           # YOND_SIDD.py:503-505
                p['scale'] = (p['wp'] - p['bl']) / p['ratio']
                return p

            def account(k, data, res):
                psnrs, ssims = [], []
                psnrs_ic, ssims_ic, ic_gains, ic_cfa = [], [], [], []
                if data.get('hr') is not None:
                    hr = data['hr'] if isinstance(data['hr'], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data['hr'], np.float32)).to(self.device)
                    H, W = hr.shape
                    for dn in res['raw_dns']:
                        ps, ss = P.block_metrics(dn, hr.clamp(0, 1), bh=H, bw=W)          # whole-frame PSNR / SSIM (data range 1)
                        psnrs.append(float(np.mean(ps)))
                        ssims.append(float(np.mean(ss)))
                    sums.update(psnrs, ssims)
                    if ic_sums is not None:
                        target = hr.clamp(0, 1)                      # (the clamp is what makes a saturated target exactly 1: left out of the gain)
                        for it, dn in enumerate(res['raw_dns']):
                            corrected, dev_sums = IL.illuminance_correct(dn, target, mode=self.illum_corr, clip=True)
                            total, per_cfa, den, count = IL.gains(dev_sums)
                            if den == 0 or count == 0 or not np.isfinite(total) or (self.illum_corr == 'cfa' and not np.isfinite(per_cfa).all()):
                                log(f"[rank {self.rank}] warning: {data['name']} round {it}: no illuminance gain (sum p^2 = {den:g} over {count:g} "
                                    "unsaturated targets): reported uncorrected", self.logfile)
                                psnrs_ic.append(psnrs[it])
                                ssims_ic.append(ssims[it])
                            else:
                                ps, ss = P.block_metrics(corrected, target, bh=H, bw=W)
                                psnrs_ic.append(float(np.mean(ps)))
                                ssims_ic.append(float(np.mean(ss)))
                                if it < n_it:
                                    ic_gain_sums[2 * it] += total
                                    ic_gain_sums[2 * it + 1] += 1
                            ic_gains.append(total)
                            ic_cfa.append(per_cfa)
                        ic_sums.update(psnrs_ic, ssims_ic)
                elif ic_sums is not None and not getattr(self, '_ic_noted', False):
                    self._ic_noted = True
                    log(f"[rank {self.rank}] --illum-corr {self.illum_corr}: ignored for items without a reference frame (hr)", self.logfile)
                self.metrics[data['name']] = {'psnr': psnrs, 'ssim': ssims, 'reg': res['regs']}
                if psnrs_ic:
                    self.metrics[data['name']].update(psnr_ic=psnrs_ic, ssim_ic=ssims_ic, illum_gain=ic_gains)
                    if self.illum_corr == 'cfa':
                        self.metrics[data['name']]['illum_gain_cfa'] = ic_cfa
                true = ""
                if self.true_level is not None:
                    # the pipeline's (K, sigma) are DN of the frame it is handed (YOND_SIDD.py:356 scales by wp - bl), digital gain
                    # included: a frame exposed at 1 / ratio and scaled back by ratio carries ratio * K and ratio * SIGMA
                    ratio = float(data.get('ratio', 1))
                    K, sigma = self.true_level[0] * ratio, self.true_level[1] * ratio
                    # (SIGMA = 0, pure shot noise, has no relative error: None there, and no share in the sweep's mean)
                    rel = [(float(abs(q[0] - K) / K), float(abs(q[1] - sigma) / sigma) if sigma > 0 else None) for q in res['params']]
                    self.metrics[data['name']].update(true=(K, sigma), rel_err=rel)
                    for it, (rk, rs) in enumerate(rel[:n_it]):
                        rel_sums[4 * it] += rk
                        rel_sums[4 * it + 1] += 1
                        if rs is not None:
                            rel_sums[4 * it + 2] += rs
                            rel_sums[4 * it + 3] += 1
                    true = f", true K={K:.3f}, sigma={sigma:.3f}"
                    if self.camera_noise is not None and 'd' in self.camera_noise['code']:
                        bias = [float(v) * ratio for v in CN.dark_bias(self.camera_noise, self.camera_noise['code'])]
                        self.metrics[data['name']]['bias'] = bias
                        true += ", dark bias " + "/".join(f"{v:.3f}" for v in bias)
                kld = ""
                paired = data.get('hr') is not None and data.get('lr') is not None
                rep = self.model_kld(data, res, wp, bl) if self.noise_kld is not None and paired else None
                if rep is not None:
                    self.metrics[data['name']].update(rep)
                    kld_sums[0] += rep['kld']
                    kld_sums[1] += rep['kld_floor']
                    kld_sums[2] += 1
                    kld = f", KLD={rep['kld']:.3e} (cfa " + "/".join(f"{v:.3e}" for v in rep['kld_cfa']) + ")"
                    if len(rep['kld_bands']) > 1:
                        kld += " (bands " + "/".join(f"{v:.3e}" for v in rep['kld_bands']) + ")"
                    kld += f", KLD floor={rep['kld_floor']:.3e}"
                elif self.noise_kld is not None and paired:
                    log(f"[rank {self.rank}] warning: {data['name']}: the estimate K={res['params'][-1][0]}, sigma={res['params'][-1][1]} is not finite: no KLD",
                        self.logfile)
                elif self.noise_kld is not None and not getattr(self, '_kld_noted', False):
                    self._kld_noted = True
                    log(f"[rank {self.rank}] --noise-kld: ignored for items without a reference frame (hr)", self.logfile)
                bp = ""
                if 'bad_pixels' in data:
                    rep_bp = data['bad_pixels']
                    self.metrics[data['name']]['bad_pixels'] = {'hot': rep_bp['hot'], 'cold': rep_bp['cold']}
                    if rep_bp.get('model') is not None:
                        self.metrics[data['name']]['bad_pixels_model'] = rep_bp['model']
                    bp = f", bad pixels hot={rep_bp['hot']}, cold={rep_bp['cold']}"
                    if 'defects_truth' in data:
                        truth = {(int(r), int(c)) for r, c in data['defects_truth']}
                        got = {(int(r), int(c)) for r, c in rep_bp['points']}
                        self.metrics[data['name']]['defects'] = {'n': len(truth), 'found': len(truth & got), 'false': len(got - truth)}
                        bp += f", found {len(truth & got)} / {len(truth)} injected, {len(got - truth)} false"
                        if rep_bp['overflow']:
                            bp += f" (of the first {len(got)} coordinates)"
                elif 'defects_truth' in data:
                    self.metrics[data['name']]['defects'] = {'n': len(data['defects_truth'])}
                    bp = f", {len(data['defects_truth'])} injected defects left in"
                if 'row_noise' in data:
                    self.metrics[data['name']]['row_noise'] = dict(data['row_noise'])
                    bp += f", row noise removed sigma={data['row_noise']['sigma']:.3f}, max={data['row_noise']['max']:.3f} DN"
                    if self.camera_noise is not None and 'r' in self.camera_noise['code']:
                        bp += f" (injected sigR={float(self.camera_noise['sigR']):g})"
                ic = ""
                if psnrs_ic:
                    ic = f", PSNR(ic)={psnrs_ic[-1]:.2f}, SSIM(ic)={ssims_ic[-1]:.4f}, gain={ic_gains[-1]:.5f}"
                    if self.illum_corr == 'cfa':
                        ic += " (" + "/".join(f"{v:.5f}" for v in ic_cfa[-1]) + ")"
                log(f"[rank {self.rank}] {data['name']}: " + (f"PSNR={psnrs[-1]:.2f}, SSIM={ssims[-1]:.4f}" if psnrs else "denoised (no reference frame)") + ic
                    + f", K={res['params'][-1][0]:.3f}, sigma={res['params'][-1][1]:.3f}" + true + kld + bp, self.logfile)

            def deliver(k, data, res):
                if callable(self.on_result):
                    self.on_result(data['name'], res)
                info = {'rounds': [(float(q[0]), float(q[1])) for q in res['params']]}
                if 'bad_pixels' in data:
                    info['bad_pixels'] = {'hot': data['bad_pixels']['hot'], 'cold': data['bad_pixels']['cold']}
                    if self.bad_pixels[0] == 'auto':
                        info['bad_pixels_points'] = [[int(r), int(c)] for r, c in data['bad_pixels']['points'][:BP.MAX_SAVED_POINTS]]
                if 'row_noise' in data:
                    info['row_noise'] = dict(data['row_noise'])
                if writer is not None and ic_sums is not None:
                    # the saved frame stays uncorrected (the correction needs the ground truth); its sidecar names the last round's gain
                    account(k, data, res)
                    if 'illum_gain' in self.metrics[data['name']]:
                        info['illum_gain'] = self.metrics[data['name']]['illum_gain'][-1]
                        if self.illum_corr == 'cfa':
                            info['illum_gain_cfa'] = self.metrics[data['name']]['illum_gain_cfa'][-1]
                if writer is not None:                       # queued on this stream before the drivers reuse the buffer; written by the writer's threads
                    writer.put(data['name'], res['raw_dns'][-1], (bl, wp, data.get('ratio', 1)), info)
                if writer is None or ic_sums is None:
                    account(k, data, res)

            touch = self.bad_pixels is not None or self.synth_defects is not None or self.row_denoise is not None
            streamed = STREAM_EVAL and getattr(self.parser, 'stream', True) and not self.parser.verbose and P.stream_applies(self.pipe, self.pipe, self.biaslut)
            if streamed:
                # pipeline.denoise_stream: the estimator of the next frame on a side stream, the network passes of consecutive frames on two lanes -- every
                # frame's result is IterDenoise's (tests/test_hip_pipeline.py); results arrive a few frames late, in order
                queue = []

                def feed():
                    for k, data in loader:
                        if self.true_level is not None:
                            data = self.synthesise(data, wp, bl)
                        if touch:
                            data = self.repair(data, wp, bl)
                        if callable(self.on_input):
                            self.on_input(data['name'], data['lr'])
                        queue.append((k, data))
                        yield data['lr'], params_of(data)
                t1 = time.perf_counter()
                for res in P.denoise_stream(feed(), self.net, self.arch, self.pipe, device=self.device):
                    k, data = queue.pop(0)
                    deliver(k, data, res)
                    npix += int(np.prod(tuple(data['lr'].shape)))
                torch.cuda.synchronize()
                t_path += time.perf_counter() - t1           # (includes what the loop waited for its loader threads)
            else:
                for k, data in loader:
                    if self.true_level is not None:
                        data = self.synthesise(data, wp, bl)
                    if touch:
                        data = self.repair(data, wp, bl)
                    if callable(self.on_input):
                        self.on_input(data['name'], data['lr'])
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    res = self.IterDenoise(data, {'p': params_of(data), 'img_id': k})
                    deliver(k, data, res)
                    torch.cuda.synchronize()
                    t_path += time.perf_counter() - t1
                    npix += int(np.prod(tuple(data['lr'].shape)))
            torch.cuda.synchronize()
            dt = D.max_over_ranks(time.perf_counter() - t0, self.device)
            red = sums.reduce(self.device)
            ic_gain = []
            if ic_sums is not None:
                # one more all-reduce, only with --illum-corr: the corrected meters (MetricSums' layout: [psnr, ssim] per round, the last
                # round's, the count) and, behind them, per round [sum of the total gains, frames that had one]
                v = D.sum_over_ranks(ic_sums.vec.tolist() + ic_gain_sums, self.device)
                cnt, base = v[2 * (n_it + 1)], 2 * (n_it + 1) + 1
                if cnt:
                    for it in range(n_it):
                        red[f'psnr_ic_iter{it}'], red[f'ssim_ic_iter{it}'] = v[2 * it] / cnt, v[2 * it + 1] / cnt
                    red['psnr_ic_last'], red['ssim_ic_last'] = v[2 * n_it] / cnt, v[2 * n_it + 1] / cnt
                    ic_gain = [v[base + 2 * it] / max(v[base + 2 * it + 1], 1) for it in range(n_it)]
            if self.true_level is not None:
                rel = D.sum_over_ranks(rel_sums, self.device)
                for it in range(n_it):
                    if rel[4 * it + 1]:
                        red[f'rel_err_K_iter{it}'] = rel[4 * it] / rel[4 * it + 1]
                    if rel[4 * it + 3]:
                        red[f'rel_err_sigma_iter{it}'] = rel[4 * it + 2] / rel[4 * it + 3]
            if self.noise_kld is not None:
                v = D.sum_over_ranks(kld_sums, self.device)      # one more all-reduce, only with --noise-kld
                if v[2]:
                    red['kld'], red['kld_floor'] = v[0] / v[2], v[1] / v[2]
            results[label] = red
            if self.rank == 0:
                log(f'{self.method_name} [{label}]: {len(ds)} frames', self.logfile)
                if red['count']:
                    for it in range(n_it):
                        log(f"Iter{it}: PSNR={red[f'psnr_iter{it}']:.2f}, SSIM={red[f'ssim_iter{it}']:.4f}"
                            + (f", PSNR(ic)={red[f'psnr_ic_iter{it}']:.2f}, SSIM(ic)={red[f'ssim_ic_iter{it}']:.4f}, gain={ic_gain[it]:.5f}"
                               if f'psnr_ic_iter{it}' in red else "")
                            + (f", fit {self.fit}: mean |K_est - K| / K = {red[f'rel_err_K_iter{it}']:.4f}" if f'rel_err_K_iter{it}' in red else "")
                            + (f", mean |sigma_est - sigma| / sigma = {red[f'rel_err_sigma_iter{it}']:.4f}" if f'rel_err_sigma_iter{it}' in red else ""),
                            self.logfile)
                    log(f"Iter_last: PSNR={red['psnr_last']:.2f}, SSIM={red['ssim_last']:.4f}"
                        + (f", PSNR(ic)={red['psnr_ic_last']:.2f}, SSIM(ic)={red['ssim_ic_last']:.4f}" if 'psnr_ic_last' in red else ""), self.logfile)
                if 'kld' in red:
                    log(f"Noise model {self.noise_kld[0]}: mean KLD={red['kld']:.3e}, mean KLD floor={red['kld_floor']:.3e}", self.logfile)
                log(f"{len(ds)} frames on {self.world} GPU(s) in {dt:.2f} s (rank 0: {t_path / max(len(mine), 1) * 1e3:.1f} ms per frame in "
                    + ("denoise_stream + metrics, waits for the loader threads included" if streamed else "IterDenoise + metrics")
                    + f" = {npix / 1e6 / max(t_path, 1e-9):.0f} Bayer MP/s" + ("" if streamed else "; the rest is data loading") + ")", self.logfile)
        if self.rank == 0:
            log(f"collectives: backend={D.STATS['backend']}, all_reduce={D.STATS['all_reduce']}, barrier={D.STATS['barrier']}", self.logfile)
        return results


def main(argv=None):
    trainer = YOND_Full(argv)
    try:
        return trainer.eval(-1)
    finally:
        D.finalize()


if __name__ == '__main__':
    main()
