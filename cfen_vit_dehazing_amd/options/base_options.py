"""Command-line flags of the inference harness, same names / types / defaults as the reference's
options/base_options.py:8-250 for every flag the v3 path reads (SURVEY 5 "Config / flags"), plus the
harness flags of test.py.  Differences, all stated here:
  * --model / --model_G / --dataset_mode default to the values that actually reach the v3 generator
    (`dec_vit`, `iid_hlgvit_crs_gd4_cfs_v3`, `dec_vit`); the reference's defaults (`vit`,
    `iid_hlgvit_crs_gd4`, `vit`) select modules that do not import, so its README commands
    only work once these three are given.  Passing them explicitly works as in the reference.
  * --hidden_dim_ratio / --n_feats keep the reference defaults (6 / 32); the released checkpoints need
    `--n_feats 24 --hidden_dim_ratio 4|2` exactly as in the README.
  * --precision single|half (reference flag, base_options.py:114, unused there) selects the HIP compute
    type: fp32 MFMA or fp16 storage with fp32 accumulation.
  * flags of the training / IPT leftovers are accepted and ignored (parse_known_args), with a note.
"""
import argparse
import os

import torch

from .. import resample as _resample
from ..util import util


class BaseOptions():
    def __init__(self):
        self.parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
        self.initialized = False

    def initialize(self):
        p = self.parser
        p.add_argument('--dataroot', required=True, help='path to images (should have subfolder hazy)')
        p.add_argument('--batchSize', type=int, default=1, help='input batch size')
        p.add_argument('--loadSize', type=int, default=256, help='edge of the half-resolution feature map (image edge / 2)')
        p.add_argument('--fineSize', type=int, default=128)
        p.add_argument('--input_nc', type=int, default=3)
        p.add_argument('--output_nc', type=int, default=3)
        p.add_argument('--model_G', type=str, default='iid_hlgvit_crs_gd4_cfs_v3', help='selects model to use for netG')
        p.add_argument('--gpu_ids', type=str, default='0', help='gpu ids: e.g. 0  0,1,2. use -1 for CPU (unsupported by the HIP path)')
        p.add_argument('--name', type=str, default='experiment_name', help='checkpoint directory name under --checkpoints_dir')
        p.add_argument('--dataset_mode', type=str, default='dec_vit')
        p.add_argument('--model', type=str, default='dec_vit')
        p.add_argument('--which_direction', type=str, default='AtoB')
        p.add_argument('--nThreads', default=0, type=int, help='# threads for loading data')
        p.add_argument('--checkpoints_dir', type=str, default='./checkpoints', help='models are saved here')
        p.add_argument('--sb', action='store_true', help='take images in order (otherwise randomly, as the reference does)')
        p.add_argument('--display_winsize', type=int, default=256)
        p.add_argument('--max_dataset_size', type=int, default=float("inf"))
        p.add_argument('--resize_or_crop', type=str, default='resize',
                       help="the reference default 'resize' matches no branch of get_transform: images are fed at native size")
        p.add_argument('--init_type', type=str, default='kaiming', help='network initialization [normal|xavier|kaiming|orthogonal]')
        p.add_argument('--verbose', action='store_true')
        p.add_argument('--suffix', default='', type=str)
        p.add_argument('--out_all', action='store_true', help='keep only the dehazed image (fake_A) among the outputs')
        p.add_argument('--seed', type=int, default=1)
        # transformer / generator geometry (base_options.py:96-110,191-201)
        p.add_argument('--patch_size', type=int, default=32, help='LViT window edge in feature-map pixels')
        p.add_argument('--rgb_range', type=int, default=255)
        p.add_argument('--n_colors', type=int, default=3)
        p.add_argument('--hidden_dim_ratio', type=int, default=6)
        p.add_argument('--n_feats', type=int, default=32)
        p.add_argument('--precision', type=str, default='single', choices=('single', 'half'),
                       help='HIP compute type: single = fp32 MFMA, half = fp16 storage / fp32 accumulate')
        p.add_argument('--no_half_guard', action='store_true',
                       help='(extension) with --precision half the first batch also runs in fp32 once and the model falls back to single when the '
                            'fp16 outputs differ by more than 1.5e-2 (range safety of a real checkpoint); this flag skips that check')
        p.add_argument('--half_guard_every', type=int, default=32,
                       help='(extension) with --precision half, repeat that fp32 comparison on every N-th batch of the run (0 = first batch only); all '
                            'ranks of a sharded run agree on the outcome, and the batches since the last passed check are redone in fp32 after a failure')
        p.add_argument('--in_flight', type=int, default=1,
                       help='(extension) batches kept in flight by test.py: 1 = the reference loop (set_input / test / save, one at a time); K > 1 = '
                            'the pipelined driver (cfen_vit_dehazing_amd/pipeline.py): K launch-plan replicas replayed from hipGraphs on K streams, pinned '
                            'asynchronous copies both ways, PNG decode in the DataLoader workers (--nThreads) and encode in --writers threads; the files '
                            'written are byte-identical to the sequential loop')
        p.add_argument('--writers', type=int, default=8, help='(extension) PNG encoder threads of the pipelined driver')
        p.add_argument('--png_compress_level', type=int, default=-1,
                       help='(extension) zlib level 0..9 of the result PNGs; -1 (default) = PIL\'s own default, the reference\'s files byte for byte. 1 encodes ~3x faster '
                            '(same pixels, larger files)')
        p.add_argument('--writer_procs', type=int, default=0,
                       help='(extension) PNG encoder PROCESSES of the pipelined driver instead of --writers threads (0 = threads): forked right after option parsing, images '
                            'handed over through shared memory; encode scales with the host cores (threads contend for the GIL around the compressor)')
        p.add_argument('--gpu_png', action='store_true',
                       help='(extension) encode the result PNGs on the device (cfen_vit_dehazing_amd/png.py: per-strip filtering and Huffman coding, no LZ77): '
                            'the same pixels in larger files that are not byte-identical to PIL\'s; the host only adds the container and its CRC. Not with '
                            '--writer_procs or --png_compress_level')
        p.add_argument('--u8_input', action='store_true',
                       help='(extension) the dataset hands over uint8 HWC images and ToTensor + Normalize(0.5, 0.5) run on the device '
                            'inside the generator launch plan (12x fewer bytes over PCIe); results are identical')
        p.add_argument('--tile', action='store_true',
                       help='(extension) dehaze images of any size: overlapping image_size x image_size tiles through the fixed-size generator, blended '
                            'back to the input size (cfen_vit_dehazing_amd/tiled.py); needs --batchSize 1 and --in_flight 1')
        p.add_argument('--tile_overlap', type=int, default=None, help='(extension) --tile: overlap of neighbouring tiles in pixels (default image_size // 8)')
        p.add_argument('--tile_batch', type=int, default=8, help='(extension) --tile: tiles per forward')
        p.add_argument('--tile_pack', type=int, default=1,
                       help='(extension) --tile: run N consecutive images as one group whose tiles share full --tile_batch forwards '
                            '(tiled.dehaze_tiled_many): a folder of small images runs ceil(tiles / tile_batch) forwards per group instead of at least '
                            'one short forward per image; same files, names and metrics rows; 1 = one image at a time')
        p.add_argument('--fit', action='store_true',
                       help='(extension) dehaze images of any size in ONE forward: every image is resampled to image_size x image_size on the device '
                            '(PIL\'s Image.resize byte for byte, cfen_vit_dehazing_amd/fit.py; the aspect ratio is not kept), run through the unchanged '
                            'generator, and the outputs are resampled back to the input size; --batchSize N for equal-sized images; not with --tile, '
                            'needs --in_flight 1 and --resize_or_crop resize | none')
        p.add_argument('--fit_filter', type=str, default='bicubic', choices=_resample.FILTERS,
                       help='(extension) --fit: the resampling filter, both ways (the reference resizes with Image.BICUBIC everywhere)')
        p.add_argument('--fit_refine', type=str, default='none', choices=('none', 'guided'),
                       help='(extension) --fit: how the dehazed image comes back to the input size. none: the resampling filter, as for the other '
                            'outputs. guided: guided upsampling (He & Sun, "Fast Guided Filter") -- a local linear model between the resampled hazy '
                            'bytes and the dehazed output is fitted at image_size x image_size, smoothed, upsampled and applied to the FULL-resolution '
                            'hazy image, which supplies the detail (cfen_vit_dehazing_amd/fit.py, include/cfen_guided.h); the other outputs keep the filter')
        p.add_argument('--fit_radius', type=int, default=2,
                       help='(extension) --fit_refine guided: radius of the (2 r + 1)^2 window at image_size x image_size, 1 .. 16. The defaults of '
                            '--fit_radius and --fit_eps come from a synthetic scattering-model experiment (DESIGN section 14), not from a checkpoint')
        p.add_argument('--fit_eps', type=float, default=1e-4,
                       help='(extension) --fit_refine guided: regulariser of the local variance, in squared units of the [0, 1] intensity scale, > 0')
        p.add_argument('--self_ensemble', action='store_true',
                       help='(extension; the reference accepts the flag, base_options.py:133, and never acts on it) geometric self-ensemble: every image '
                            'runs as its eight flips / transposes in one batch-8 forward and the outputs, mapped back, are averaged on the device '
                            '(cfen_vit_dehazing_amd/ensemble.py; the reference\'s Model.forward_x8, models/vit_model.py:102-147); 8x the forward time; '
                            'needs --in_flight 1')
        p.add_argument('--eval', action='store_true',
                       help='(extension) score every dehazed image against its ground truth on the device: per-image PSNR (RGB, 10 log10(1 / MSE)) and SSIM '
                            '(the reference\'s pytorch_msssim.ssim, 11 x 11 Gaussian window, valid convolution) of the very bytes written to the PNG, into '
                            'results/<name>/<phase>_<epoch>/metrics.csv; needs --sb and --in_flight 1')
        p.add_argument('--eval_metrics', type=str, default=None,
                       help='(extension) --eval: the columns of metrics.csv, psnr,ssim (default) or psnr,ssim,msssim. msssim is the reference\'s '
                            'pytorch_msssim.msssim (five levels of 2 x 2 means, normalize=None: nan where a level is anticorrelated), scored on the device '
                            'in the same call; every image must be at least 176 pixels on a side')
        p.add_argument('--eval_ciede2000', action='store_true',
                       help='(extension) --eval: a last column ciede2000 in metrics.csv, the mean CIEDE2000 colour difference (Sharma, Wu and Dalal 2005, '
                            'kL = kC = kH = 1) of the written bytes against the ground truth, both read as sRGB; scored on the device in one more call '
                            'per batch')
        p.add_argument('--eval_noref', action='store_true',
                       help='(extension) score without ground truth: statistics of every hazy image and of its dehazed output side by side -- mean '
                            'dark channel (He, Sun and Tang 2009), entropy, average gradient and contrast of the luma, and the share of newly '
                            'saturated pixels (sigma of Hautiere et al. 2008) -- from the very bytes written to the PNG, on the device, into '
                            'results/<name>/<phase>_<epoch>/noref.csv; needs --sb and --in_flight 1, does not need --eval, clear/ or --gt_dir')
        p.add_argument('--noref_radius', type=int, default=None,
                       help='(extension) --eval_noref: radius of the dark channel\'s (2 r + 1)^2 window, 0 .. 16 (default 7: He, Sun and Tang\'s 15 x 15)')
        p.add_argument('--gt_dir', type=str, default=None,
                       help='(extension) --eval: folder of ground-truth images, paired by stem or by the stem up to its first "_" (default <dataroot>/clear)')
        p.add_argument('--patch_dim', type=int, default=2)
        p.add_argument('--num_heads', type=int, default=4)
        p.add_argument('--num_layers', type=int, default=1)
        p.add_argument('--dropout_rate', type=float, default=0)
        p.add_argument('--no_norm', action='store_true')
        p.add_argument('--no_mlp', action='store_true')
        p.add_argument('--pos_every', action='store_true')
        p.add_argument('--no_pos', action='store_true')
        p.add_argument('--num_queries', type=int, default=1)
        self.initialized = True

    def parse(self, argv=None):
        if not self.initialized:
            self.initialize()
        opt, unknown = self.parser.parse_known_args(argv)
        if unknown:
            print('note: ignoring flags outside the inference path: %s' % ' '.join(unknown))
        opt.isTrain = self.isTrain
        str_ids = opt.gpu_ids.split(',')
        opt.gpu_ids = []
        for str_id in str_ids:
            id = int(str_id)
            if id >= 0:
                opt.gpu_ids.append(id)
        # one process per GPU: under `python -m torch.distributed.run --nproc-per-node N test.py ...` every rank takes the GPU of its
        # LOCAL_RANK (whatever --gpu_ids says) and its own slice of the dataset; the reference's counterpart is nn.DataParallel over
        # --gpu_ids (networks_iid_hlgvit_crs_gd4_cfs_v3.py:77-83)
        from ..parallel import dist_env
        opt.dist_rank, opt.dist_world, local = dist_env()
        if opt.dist_world > 1:
            if opt.gpu_ids != [local]:
                print('[rank %d] torch.distributed.run: --gpu_ids %s overridden by LOCAL_RANK -> GPU %d' % (opt.dist_rank, opt.gpu_ids, local))
            opt.gpu_ids = [local]
        if opt.in_flight < 1:
            raise ValueError('--in_flight must be >= 1')
        if getattr(opt, 'tile', False):
            if opt.batchSize != 1 or opt.in_flight != 1:
                raise ValueError('--tile runs one image at a time through the sequential loop: it needs --batchSize 1 and --in_flight 1 '
                                 '(got --batchSize %d --in_flight %d)' % (opt.batchSize, opt.in_flight))
            if opt.tile_batch < 1:
                raise ValueError('--tile_batch must be >= 1')
        if getattr(opt, 'fit', False):
            if getattr(opt, 'tile', False):
                raise ValueError('--fit and --tile are two answers to the same question (one resampled forward, or overlapping tiles): give one of them')
            if opt.in_flight != 1:
                raise ValueError('--fit runs through the sequential loop: it needs --in_flight 1 (got --in_flight %d); the pipelined driver '
                                 'replays plain forwards only' % opt.in_flight)
            if opt.resize_or_crop not in ('resize', 'none'):
                raise ValueError('--fit resamples the decoded image itself: it needs --resize_or_crop resize | none (got --resize_or_crop %s, '
                                 'which resizes in the loader)' % opt.resize_or_crop)
        if getattr(opt, 'fit_refine', 'none') != 'none' and not getattr(opt, 'fit', False):
            raise ValueError('--fit_refine chooses how --fit brings the dehazed image back to the input size: it needs --fit')
        if getattr(opt, 'fit_refine', 'none') != 'none':
            if not 1 <= opt.fit_radius <= 16:
                raise ValueError('--fit_refine guided: --fit_radius must be in 1 .. 16 (got --fit_radius %d)' % opt.fit_radius)
            if not (opt.fit_eps > 0 and opt.fit_eps != float('inf')):
                raise ValueError('--fit_refine guided: --fit_eps must be finite and > 0 (got --fit_eps %r)' % opt.fit_eps)
        if getattr(opt, 'tile_pack', 1) < 1:
            raise ValueError('--tile_pack must be >= 1')
        if getattr(opt, 'tile_pack', 1) > 1:
            if not getattr(opt, 'tile', False):
                raise ValueError('--tile_pack packs the tiles of several images into common batches: it needs --tile')
            if opt.in_flight != 1:
                raise ValueError('--tile_pack runs through the sequential loop: it needs --in_flight 1 (got --in_flight %d)' % opt.in_flight)
        if getattr(opt, 'self_ensemble', False) and opt.in_flight != 1:
            raise ValueError('--self_ensemble runs through the sequential loop: it needs --in_flight 1 (got --in_flight %d); the pipelined driver '
                             'replays plain forwards only' % opt.in_flight)
        if getattr(opt, 'eval', False):
            if opt.in_flight != 1:
                raise ValueError('--eval scores the images of the sequential loop: it needs --in_flight 1 (got --in_flight %d); the pipelined driver '
                                 'does not compute metrics' % opt.in_flight)
            if not opt.sb:
                raise ValueError('--eval needs --sb: without it the images are sampled randomly (dec_vit_data.py:51-58) and metrics.csv would not '
                                 'cover the dataset in order')
        eval_metrics_given = getattr(opt, 'eval_metrics', None) is not None
        if eval_metrics_given and not getattr(opt, 'eval', False):
            raise ValueError('--eval_metrics names the columns of --eval\'s metrics.csv: it needs --eval')
        if getattr(opt, 'eval_ciede2000', False) and not getattr(opt, 'eval', False):
            raise ValueError('--eval_ciede2000 adds a column to --eval\'s metrics.csv: it needs --eval')
        noref_radius_given = getattr(opt, 'noref_radius', None) is not None
        if noref_radius_given and not getattr(opt, 'eval_noref', False):
            raise ValueError('--noref_radius is the window of --eval_noref\'s dark channel: it needs --eval_noref')
        if getattr(opt, 'eval_noref', False):
            if opt.in_flight != 1:
                raise ValueError('--eval_noref scores the images of the sequential loop: it needs --in_flight 1 (got --in_flight %d); the pipelined '
                                 'driver does not compute metrics' % opt.in_flight)
            if not opt.sb:
                raise ValueError('--eval_noref needs --sb: without it the images are sampled randomly (dec_vit_data.py:51-58) and noref.csv would '
                                 'not cover the dataset in order')
            if noref_radius_given and not 0 <= opt.noref_radius <= 16:
                raise ValueError('--eval_noref: --noref_radius must be in 0 .. 16 (got --noref_radius %d)' % opt.noref_radius)
        opt.noref_radius = opt.noref_radius if noref_radius_given else 7
        from .. import metrics as _metrics
        opt.eval_metrics =','.join(_metrics.parse_columns(opt.eval_metrics if eval_metrics_given else 'psnr,ssim'))
        if not -1 <= opt.png_compress_level <= 9:
            raise ValueError('--png_compress_level must be -1 (PIL default) or 0..9')
        from .. import png as _png
        _png.check_options(opt)
        from ..util import util as _util
        _util.PNG_COMPRESS_LEVEL = None if opt.png_compress_level < 0 else opt.png_compress_level      # set before any writer process is forked
        if opt.in_flight > 1:
            # the pipelined driver keeps K forwards on K streams; the HIP runtime deals a process's streams onto GPU_MAX_HW_QUEUES hardware queues
            # (default 4) and two busy streams on one queue run one behind the other (4 in flight: 2.51 ms / step on 4 queues, 2.10 on 8,
            # profiles/r04_ab_hw_queues.txt).  The harness, not the user, sets it -- here, before the first HIP call of the process (set_device below)
            os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
        if len(opt.gpu_ids) > 0 and torch.cuda.is_available():
            torch.cuda.set_device(opt.gpu_ids[0])
        args = vars(opt)
        if not getattr(opt, 'eval', False):
            args = {k: v for k, v in args.items() if k not in ('eval', 'gt_dir')}      # a run without --eval prints and records what it always did
        if not eval_metrics_given:
            args = {k: v for k, v in args.items() if k != 'eval_metrics'}              # ... and one without --eval_metrics, with --eval or not
        if not getattr(opt, 'eval_ciede2000', False):
            args = {k: v for k, v in args.items() if k != 'eval_ciede2000'}            # ... and one without --eval_ciede2000
        if not getattr(opt, 'eval_noref', False):
            args = {k: v for k, v in args.items() if k not in ('eval_noref', 'noref_radius')}      # ... and one without --eval_noref
        if not getattr(opt, 'gpu_png', False):
            args = {k: v for k, v in args.items() if k != 'gpu_png'}                   # ... and so does one without --gpu_png
        if not getattr(opt, 'self_ensemble', False):
            args = {k: v for k, v in args.items() if k != 'self_ensemble'}             # ... and one without --self_ensemble
        if getattr(opt, 'tile_pack', 1) == 1:
            args = {k: v for k, v in args.items() if k != 'tile_pack'}                 # ... and one without --tile_pack
        if not getattr(opt, 'fit', False):
            args = {k: v for k, v in args.items() if k not in ('fit', 'fit_filter')}   # ... and one without --fit
        if getattr(opt, 'fit_refine', 'none') == 'none':
            args = {k: v for k, v in args.items() if k not in ('fit_refine', 'fit_radius', 'fit_eps')}   # ... and one without --fit_refine
        if opt.dist_rank == 0:
            print('------------ Options -------------')
            for k, v in sorted(args.items()):
                print('%s: %s' % (str(k), str(v)))
            print('-------------- End ----------------')
        if opt.suffix:
            suffix = ('_' + opt.suffix.format(**vars(opt))) if opt.suffix != '' else ''
            opt.name = opt.name + suffix
        expr_dir = os.path.join(opt.checkpoints_dir, opt.name)
        util.mkdirs(expr_dir)
        if opt.dist_rank == 0:
            with open(os.path.join(expr_dir, 'opt.txt'), 'wt') as opt_file:
                opt_file.write('------------ Options -------------\n')
                for k, v in sorted(args.items()):
                    opt_file.write('%s: %s\n' % (str(k), str(v)))
                opt_file.write('-------------- End ----------------\n')
        self.opt = opt
        return self.opt
