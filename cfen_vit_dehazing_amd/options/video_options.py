"""Flags of dehaze_video.py: every flag of test.py (TestOptions, unchanged) plus the stream's own.  Differences from test.py, all stated here:
  * --dataroot is not needed (there is no folder of images) and --sb is implied: frames are taken in order.
  * --batchSize defaults to 8 frames per forward, and --tile takes any --batchSize: the tiles of a batch's frames are packed into common
    forwards (hipnet.forward_tiled_many), which test.py reaches through --tile_pack.
  * --u8_input is always on: the converted frames are bytes.
  * --in_flight stays 1: the loop has its own reader and writer threads (--video_buffers).
  * --video_depth auto lets a stream of 9 to 16 bits per sample in (the float route of video.run); the default, 8, refuses it as always.
  * --eval_gt CLEAR.y4m scores the stream that leaves against a ground-truth stream of the same geometry.
  * the options are recorded in <checkpoints_dir>/<name>/video_opt.txt; opt.txt, which test.py writes, is left as it was."""
import os

from .test_options import TestOptions


class VideoOptions(TestOptions):
    def initialize(self):
        TestOptions.initialize(self)
        p = self.parser
        p.add_argument('--in', dest='video_in', required=True, help='the .y4m stream to dehaze: a path, or - for stdin')
        p.add_argument('--out', dest='video_out', required=True, help='where the dehazed .y4m stream goes: a path, or - for stdout (everything printed then goes to stderr)')
        p.add_argument('--video_matrix', default='auto', choices=('auto', 'bt601', 'bt709'),
                       help='YCbCr matrix of the stream; auto: bt709 for frames of 720 rows or more, bt601 below (a y4m header does not say)')
        p.add_argument('--video_range', default='auto', choices=('auto', 'limited', 'full'),
                       help='sample range of the stream; auto: the XCOLORRANGE tag of the header, limited (16 .. 235) without one')
        p.add_argument('--video_depth', default='8', choices=('8', 'auto'),
                       help='(extension) bits per sample the stream may have: 8 refuses every deeper stream, as always; auto reads the depth of the '
                            "header's C tag (C420p10, C444p12, Cmono16, ...: 9 to 16 bits) and takes such a stream through the float route "
                            '(DESIGN section 23), which has no --fit, --temporal, --eval_noref or --eval_flicker yet. An 8-bit stream runs as without the flag')
        p.add_argument('--video_buffers', type=int, default=4, help='slots of the ring of pinned host buffers between the reader, the device and the writer (each holds a batch both ways)')
        p.add_argument('--noref_csv', type=str, default=None, help='--eval_noref: where noref.csv goes (default: beside --out; required when --out is -)')
        p.add_argument('--temporal', action='store_true',
                       help='(extension) temporal stabilisation: smooth the local affine model out ~ a * hazy + b of neighbouring frames over time and '
                            'correct each dehazed frame by the change of its coefficients (DESIGN section 18); the first frame passes unchanged')
        p.add_argument('--temporal_strength', type=float, default=None,
                       help='--temporal: weight of the past in the recursion, in [0, 1) (default 0.8); 0 leaves every frame as the generator wrote it')
        p.add_argument('--temporal_motion', type=float, default=None,
                       help='--temporal: mean absolute change of the hazy bytes over the window, in levels, at which the recursion is switched off '
                            '(default 8.0), finite and > 0. The defaults of the --temporal options come from a synthetic scattering-model experiment '
                            '(DESIGN section 18), not from a checkpoint')
        p.add_argument('--temporal_radius', type=int, default=None, help='--temporal: radius of the (2 r + 1)^2 window at the working resolution, 1 .. 16 (default 2)')
        p.add_argument('--temporal_eps', type=float, default=None,
                       help='--temporal: regulariser of the local variance, in squared units of the [0, 1] intensity scale, finite and > 0 (default 1e-4)')
        p.add_argument('--temporal_down', type=str, default=None,
                       help='--temporal: integer factor >= 1 between the frame and the working resolution, or auto = ceil(max(H, W) / 1024) (default auto)')
        p.add_argument('--temporal_mc', type=int, default=None,
                       help='--temporal: motion compensation (DESIGN section 20): look every block of the working-resolution frame up in the previous '
                            'frame within +-N pixels, N in 0 .. 16, and let the recursion follow it, so that a moving camera no longer switches the '
                            'recursion off (default 0 = off; 8 covers a pan of 8 working-resolution pixels per frame)')
        p.add_argument('--temporal_mc_block', type=int, default=None, choices=(8, 16, 32),
                       help='--temporal_mc: edge of the matched blocks at the working resolution (default 16)')
        p.add_argument('--temporal_mc_bias', type=int, default=None,
                       help='--temporal_mc: preference for short vectors, in sixteenths of a level of mean absolute difference per pixel of displacement, '
                            '0 .. 255 (default 4). The defaults of the --temporal_mc options come from a synthetic panning experiment on the '
                            'scattering-model scene (DESIGN section 20), not from a checkpoint')
        p.add_argument('--temporal_mc_subpel', type=int, default=None, choices=(1, 2, 4),
                       help='--temporal_mc: refine the block vectors to 1/2 or 1/4 of a working-resolution pixel and fetch the previous frame and '
                            'the state bilinearly (DESIGN section 25): the working resolution is 1 / --temporal_down of the frame, so a real pan '
                            'is a fraction of a working pixel there (default 1 = whole pixels, the run without the flag). The evidence is the '
                            'synthetic panning experiment of DESIGN section 25 on the scattering-model scene, not footage')
        p.add_argument('--eval_flicker', action='store_true',
                       help='(extension) score the flicker of the stream along the motion (DESIGN section 22): per frame pair, how much the '
                            "network's frames and the frames that leave change where the hazy input, followed along block vectors, did not; "
                            'writes flicker.csv and prints one summary line. The stream itself is unchanged')
        p.add_argument('--flicker_range', type=int, default=None,
                       help='--eval_flicker: the blocks are looked up within +-N working-resolution pixels, N in 0 .. 16 (default 8; 0 compares '
                            'every pixel with the same pixel of the previous frame)')
        p.add_argument('--flicker_block', type=int, default=None, choices=(8, 16, 32), help='--eval_flicker: edge of the matched blocks (default 16)')
        p.add_argument('--flicker_bias', type=int, default=None,
                       help='--eval_flicker: preference of the search for short vectors, as --temporal_mc_bias, 0 .. 255 (default 4)')
        p.add_argument('--flicker_tol', type=int, default=None,
                       help='--eval_flicker: a pixel counts where the hazy bytes changed by at most this many levels per channel on average along '
                            'its vector, 0 .. 255 (default 8)')
        p.add_argument('--flicker_down', type=str, default=None,
                       help='--eval_flicker: integer factor >= 1 between the frame and the working resolution, or auto = ceil(max(H, W) / 1024) (default auto)')
        p.add_argument('--flicker_csv', type=str, default=None, help='--eval_flicker: where flicker.csv goes (default: beside --out; required when --out is -)')
        p.add_argument('--eval_gt', type=str, default=None, metavar='CLEAR.y4m',
                       help='(extension) score the stream that leaves against this ground-truth .y4m file (DESIGN section 24): per frame PSNR '
                            'and SSIM of the Y, Cb and Cr planes on the samples as stored, and a temporal error; writes gt.csv and prints one '
                            'summary line. The file must have the size, the C tag and the interlacing of --in and at least as many frames; - is '
                            'refused. Works on every route, 8-bit and deep. The stream itself is unchanged')
        p.add_argument('--gt_csv', type=str, default=None, help='--eval_gt: where gt.csv goes (default: beside --out; required when --out is -)')
        for a in p._actions:
            if a.dest == 'dataroot':
                a.required = False
        p.set_defaults(batchSize=8, dataroot='')

    TEMPORAL = ('strength', 'motion', 'radius', 'eps', 'down')

    @staticmethod
    def _without_temporal(text):
        """a run without --temporal prints and records what it always did"""
        return ''.join(l for l in text.splitlines(True) if not l.startswith('temporal'))

    @staticmethod
    def _without_temporal_mc(text):
        """a run without --temporal_mc prints and records what it always did"""
        return ''.join(l for l in text.splitlines(True) if not l.startswith('temporal_mc'))

    @staticmethod
    def _without_temporal_mc_subpel(text):
        """a run without --temporal_mc_subpel 2 or 4 prints and records what it always did"""
        return ''.join(l for l in text.splitlines(True) if not l.startswith('temporal_mc_subpel'))

    @staticmethod
    def _check_temporal_mc_subpel(first):
        """the refusals of --temporal_mc_subpel (what is none of 1, 2, 4 argparse itself refuses, with 2)"""
        if first.temporal_mc_subpel is None:
            return
        if not first.temporal:
            raise ValueError('--temporal_mc_subpel only applies with --temporal')
        if not first.temporal_mc:
            raise ValueError('--temporal_mc_subpel refines the vectors of --temporal_mc: it only applies with --temporal_mc > 0')

    def _check_temporal_mc(self, first):
        """the refusals of the --temporal_mc options; returns the defaults of those not given, as arguments"""
        from .. import temporal
        given = {k: getattr(first, 'temporal_' + k) for k in ('mc', 'mc_block', 'mc_bias') if getattr(first, 'temporal_' + k) is not None}
        if not first.temporal:
            if given:
                raise ValueError('%s only applies with --temporal' % ', '.join('--temporal_' + k for k in given))
            return []
        mc = given.get('mc', temporal.MC_DEFAULTS['range'])
        if not 0 <= mc <= 16:
            raise ValueError('--temporal_mc must be an integer in 0 .. 16 (0 = off), got %d' % mc)
        if mc == 0 and len(given) > ('mc' in given):
            raise ValueError('%s only applies with --temporal_mc > 0' % ', '.join('--temporal_' + k for k in given if k != 'mc'))
        try:
            temporal.check_mc_params(mc, given.get('mc_block', temporal.MC_DEFAULTS['block']), given.get('mc_bias', temporal.MC_DEFAULTS['bias']), '--temporal')
        except ValueError as e:
            raise ValueError(str(e).replace('--temporal: ', '--temporal_', 1))
        defaults = {'mc': temporal.MC_DEFAULTS['range'], 'mc_block': temporal.MC_DEFAULTS['block'], 'mc_bias': temporal.MC_DEFAULTS['bias']}
        return [a for k in defaults if k not in given for a in ('--temporal_' + k, str(defaults[k]))]

    @staticmethod
    def _without_video_depth(text):
        """a run without --video_depth prints and records what it always did"""
        return ''.join(l for l in text.splitlines(True) if not l.startswith('video_depth'))

    FLICKER = ('range', 'block', 'bias', 'tol', 'down')

    @staticmethod
    def _without_flicker(text):
        """a run without --eval_flicker prints and records what it always did"""
        return ''.join(l for l in text.splitlines(True) if not l.startswith(('eval_flicker', 'flicker_')))

    def _check_flicker(self, first):
        """the refusals of the --flicker options; returns the defaults of those not given, as arguments"""
        from .. import flicker
        given = {k: getattr(first, 'flicker_' + k) for k in self.FLICKER + ('csv',) if getattr(first, 'flicker_' + k) is not None}
        if not first.eval_flicker:
            if given:
                raise ValueError('%s only applies with --eval_flicker' % ', '.join('--flicker_' + k for k in given))
            return []
        if first.video_out == '-' and 'csv' not in given:
            raise ValueError('--eval_flicker with --out -: say where flicker.csv goes with --flicker_csv PATH')
        values = dict(flicker.DEFAULTS, **{k: v for k, v in given.items() if k != 'csv'})
        if values['down'] != 'auto':
            if not values['down'].isdigit() or int(values['down']) < 1:
                raise ValueError("--flicker_down must be auto or an integer >= 1 (got --flicker_down %s)" % values['down'])
            values['down'] = int(values['down'])
        try:
            flicker.check_params(values['range'], values['block'], values['bias'], values['tol'], values['down'], '--flicker')
        except ValueError as e:
            raise ValueError(str(e).replace('--flicker: ', '--flicker_', 1))
        return [a for k in self.FLICKER if k not in given for a in ('--flicker_' + k, str(flicker.DEFAULTS[k]))]

    @staticmethod
    def _without_gt(text):
        """a run without --eval_gt prints and records what it always did"""
        return ''.join(l for l in text.splitlines(True) if not l.startswith(('eval_gt', 'gt_csv')))

    @staticmethod
    def _check_gt(first):
        """the refusals of --eval_gt and --gt_csv; with an input FILE the two headers are compared here, so that a ground truth of another
        geometry is refused at parsing (a pipe: video.run compares as soon as it has read the input's header)"""
        if not first.eval_gt:
            if first.gt_csv:
                raise ValueError('--gt_csv is where --eval_gt writes: it needs --eval_gt')
            return
        if first.eval_gt == '-':
            raise ValueError('--eval_gt takes a .y4m file: - (stdin) is refused, it is where --in - reads the hazy stream')
        if first.video_out == '-' and not first.gt_csv:
            raise ValueError('--eval_gt with --out -: say where gt.csv goes with --gt_csv PATH')
        from .. import video
        max_depth = 16 if first.video_depth == 'auto' else 8
        gt = video.peek_header(first.eval_gt, max_depth)          # OSError (a ValueError to the caller below) or Y4MError: the run ends here
        if first.video_in != '-':
            try:
                src = video.peek_header(first.video_in, max_depth)
            except (OSError, video.Y4MError):
                return                                            # video.run says what is wrong with the input
            video.check_gt_header(src, gt, first.eval_gt)

    def _check_temporal(self, first):
        """the refusals of the --temporal options; returns the defaults of those not given, as arguments"""
        from .. import temporal
        given = {k: getattr(first, 'temporal_' + k) for k in self.TEMPORAL if getattr(first, 'temporal_' + k) is not None}
        if not first.temporal:
            if given:
                raise ValueError('%s only applies with --temporal' % ', '.join('--temporal_' + k for k in given))
            return []
        values = dict(temporal.DEFAULTS, **given)
        if values['down'] != 'auto':
            if not values['down'].isdigit() or int(values['down']) < 1:
                raise ValueError("--temporal_down must be auto or an integer >= 1 (got --temporal_down %s)" % values['down'])
            values['down'] = int(values['down'])
        try:
            temporal.check_params(values['radius'], values['eps'], values['strength'], values['motion'], values['down'], '--temporal')
        except ValueError as e:
            raise ValueError(str(e).replace('--temporal: ', '--temporal_', 1))
        return [a for k in self.TEMPORAL if k not in given for a in ('--temporal_' + k, repr(temporal.DEFAULTS[k]) if k != 'down' else 'auto')]

    def parse(self, argv=None):
        import sys
        if not self.initialized:
            self.initialize()
        argv = list(sys.argv[1:] if argv is None else argv)
        first, _ = self.parser.parse_known_args(argv)
        if first.batchSize < 1:
            raise ValueError('--batchSize must be >= 1')
        if first.video_buffers < 1:
            raise ValueError('--video_buffers must be >= 1')
        if first.in_flight != 1:
            raise ValueError('dehaze_video.py has its own reader and writer threads (--video_buffers): --in_flight stays 1')
        if first.eval_noref and first.video_out == '-' and not first.noref_csv:
            raise ValueError('--eval_noref with --out -: say where noref.csv goes with --noref_csv PATH')
        if first.noref_csv and not first.eval_noref:
            raise ValueError('--noref_csv is where --eval_noref writes: it needs --eval_noref')
        if first.video_depth == 'auto' and first.video_in != '-':
            # a file: its header is read here, so that a deep stream with a flag of the uint8 machinery is refused at parsing (a pipe: video.run
            # refuses as soon as it has read the header)
            from .. import video
            tag = video.peek_deep_tag(first.video_in)
            if tag is not None:
                video.refuse_deep_flags(first, tag)
        try:
            self._check_gt(first)
        except OSError as e:
            raise ValueError('--eval_gt %s: %s' % (first.eval_gt, e.strerror or e))
        depth_given = first.video_depth != '8'
        extra_temporal = self._check_temporal(first) + self._check_temporal_mc(first) + self._check_flicker(first)
        self._check_temporal_mc_subpel(first)
        mc_on = bool(first.temporal and first.temporal_mc)
        subpel_on = mc_on and (first.temporal_mc_subpel or 1) > 1
        # test.py's own checks run on what test.py would be given: frames in order, and --tile there means one image per call.  What that parse
        # prints and records is held back, corrected to the batch size this run really uses, and recorded in a file of its own: opt.txt stays
        # what the last test.py run of the same --name wrote
        import contextlib
        import io
        extra = ['--sb', '--u8_input'] + (['--batchSize', '1'] if first.tile else [])
        opt_txt = os.path.join(first.checkpoints_dir, first.name + (('_' + first.suffix.format(**vars(first))) if first.suffix else ''), 'opt.txt')
        before = open(opt_txt, 'rb').read() if os.path.exists(opt_txt) else None
        held = io.StringIO()
        with contextlib.redirect_stdout(held):
            opt = TestOptions.parse(self, argv + extra + extra_temporal)
        opt.batchSize = first.batchSize
        if opt.temporal and opt.temporal_down != 'auto':
            opt.temporal_down = int(opt.temporal_down)
        if opt.eval_flicker and opt.flicker_down != 'auto':
            opt.flicker_down = int(opt.flicker_down)
        text = held.getvalue().replace('\nbatchSize: 1\n', '\nbatchSize: %d\n' % opt.batchSize) if first.tile else held.getvalue()
        text = text if first.temporal else self._without_temporal(text)
        text = text if mc_on else self._without_temporal_mc(text)
        text = text if subpel_on else self._without_temporal_mc_subpel(text)
        text = text if first.eval_flicker else self._without_flicker(text)
        text = text if depth_given else self._without_video_depth(text)
        text = text if first.eval_gt else self._without_gt(text)
        sys.stdout.write(text)
        sys.stdout.flush()
        if opt.dist_rank == 0:
            try:
                recorded = open(opt_txt).read()
                recorded = recorded if first.temporal else self._without_temporal(recorded)
                recorded = recorded if mc_on else self._without_temporal_mc(recorded)
                recorded = recorded if subpel_on else self._without_temporal_mc_subpel(recorded)
                recorded = recorded if first.eval_flicker else self._without_flicker(recorded)
                recorded = recorded if depth_given else self._without_video_depth(recorded)
                recorded = recorded if first.eval_gt else self._without_gt(recorded)
                if before is None:
                    os.remove(opt_txt)
                else:
                    with open(opt_txt, 'wb') as f:
                        f.write(before)
                with open(os.path.join(os.path.dirname(opt_txt), 'video_opt.txt'), 'wt') as f:
                    f.write(recorded.replace('\nbatchSize: 1\n', '\nbatchSize: %d\n' % opt.batchSize) if first.tile else recorded)
            except OSError as e:
                print('note: could not record the options (%s)' % e)
        if opt.eval_noref and not opt.noref_csv:
            opt.noref_csv = os.path.join(os.path.dirname(os.path.abspath(opt.video_out)), 'noref.csv')
        if opt.eval_flicker and not opt.flicker_csv:
            opt.flicker_csv = os.path.join(os.path.dirname(os.path.abspath(opt.video_out)), 'flicker.csv')
        if opt.eval_gt and not opt.gt_csv:
            opt.gt_csv = os.path.join(os.path.dirname(os.path.abspath(opt.video_out)), 'gt.csv')
        return opt
