"""Frame times for decoding a sampled latent at another frame rate: plain Python lists of floats in [0, num_frames - 1],
the `times` of FlowDiffusion.decode_at / ops.latent_resample.  Time t is the instant of sampled frame t; a time between two integers is
a frame interpolated between them.  Nothing here touches torch or the device."""
import math

__all__ = ["frame_times"]


def frame_times(num_frames, factor=1, *, speed=None, reverse=False, pingpong=False):
    """Times of the output frames of a `num_frames`-frame sample.

    factor = K (int >= 1): K output frames per sampled interval - the (num_frames - 1) * K + 1 times j / K; the sampled frames
        themselves (every K-th) come back bit for bit.
    speed (float > 0, default 1): sampled frames advanced per K output frames, i.e. a step of speed / K instead of 1 / K: 0.5 is
        half-speed motion (twice the frames), 2.0 skips every other frame.  The list starts at 0 and stops at the last step that does
        not pass num_frames - 1; the end point itself is included only when a step lands on it (always, for speed = 1).
    reverse: the same times, last first.
    pingpong: forward, then back without repeating either end point (n times -> 2 n - 2), so that the list loops seamlessly.
    Every value lies in [0, num_frames - 1]: there is no extrapolation."""
    t, k = int(num_frames), int(factor)
    if t < 1:
        raise ValueError("frame_times: num_frames must be at least 1, got %r" % (num_frames,))
    if k < 1 or k != factor:
        raise ValueError("frame_times: factor must be an integer >= 1, got %r" % (factor,))
    s = 1.0 if speed is None else float(speed)
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError("frame_times: speed must be a finite number > 0, got %r" % (speed,))
    last = float(t - 1)
    if speed is None:
        n = (t - 1) * k + 1
    else:
        n = int(math.floor(last * k / s * (1.0 + 1e-12))) + 1          # (a step that lands on the end point within rounding counts)
    times = [min(j * s / k, last) for j in range(n)]
    if reverse:
        times = times[::-1]
    if pingpong and len(times) > 2:
        times = times + times[-2:0:-1]
    return times
