#!/usr/bin/env python3
"""Dehaze a YUV4MPEG2 (.y4m) stream, frame by frame, with the checkpoint and the model flags of test.py:

    python dehaze_video.py --in clip.y4m --out clear.y4m --name iid_hlgvit_crs_gd4_cfs_v3_reside --n_feats 24 \
                           --hidden_dim_ratio 4 --which_epoch 32 --fit

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python dehaze_video.py --name ... --fit --in - --out - | ffmpeg -i - out.mp4

The frame bytes go to the device as they are; YCbCr -> RGB, the forward and RGB -> YCbCr run there (cfen_vit_dehazing_amd/video.py,
include/cfen_yuv.h).  Frames of the generator's size run as they are, any other size needs --fit or --tile.  With --out - the video leaves on
stdout and everything printed goes to stderr.  --video_depth auto also takes streams of 9 to 16 bits per sample (C420p10, C444p12, ...), on a
float route (include/cfen_yuv16.h); there other sizes need --tile.  --eval_gt CLEAR.y4m scores the stream that leaves against a ground-truth
stream of the same geometry, per plane (PSNR, SSIM, a temporal error; include/cfen_planes.h), on every route, and writes gt.csv.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _video_on_stdout(argv):
    for k, a in enumerate(argv):
        if (a == '--out' and k + 1 < len(argv) and argv[k + 1] == '-') or a == '--out=-':
            return True
    return False


if __name__ == '__main__':
    log = print
    if _video_on_stdout(sys.argv[1:]):
        # keep file descriptor 1 for the video alone: a copy of it becomes the writer's target, and 1 itself, for whatever prints, becomes stderr
        sys.stdout.flush()
        video_fd = os.dup(1)
        os.dup2(2, 1)
        sys.stdout = sys.stderr
        out_file = os.fdopen(video_fd, 'wb')
    else:
        out_file = None
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    from cfen_vit_dehazing_amd import video
    try:
        opt = VideoOptions().parse()
        opt.serial_batches = True
        opt.no_flip = True
        opt.display_id = -1
        if out_file is not None:
            opt.video_out = out_file
        video.run(opt, log=log)
        if out_file is not None:
            out_file.close()
    except video.UnsafeHalfFrames as e:
        print('dehaze_video: %s' % e, file=sys.stderr)
        sys.exit(3)
    except (video.Y4MError, ValueError) as e:
        print('dehaze_video: %s' % e, file=sys.stderr)
        sys.exit(2)
    except OSError as e:
        # the consumer of the stream went away (a closed pipe), the disk is full, ...: the loop has ended and released the device
        print('dehaze_video: stopped, %s: %s' % (type(e).__name__, e), file=sys.stderr)
        try:
            if out_file is not None:
                out_file.close()
        except OSError:
            pass
        sys.exit(1)
