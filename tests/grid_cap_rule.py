"""Shapes that take the capped-grid frame kernels past their cap, and the canvas the tests put them in. ring_accumulate_kernel,
ring_subtract_kernel, air_subtract_kernel and bh_apply_kernel deal the band's lanes over at most 4096 blocks of 256 lanes and stride over
the rest (RING_ / AIR_ / BH_MAX_BLOCKS in paris_amd/csrc): 4096 x 256 = 1 048 576 lanes is the cap. A band of 1024 rows of 1025 pixels,
one pixel per lane, is 1 049 600 lanes; so is one of 4100 pixels, four per lane in 1025 groups: the last 1024 lanes are served by a
second visit of the first four blocks, whose `i / groups_x` and `i % groups_x` land in the band's final row. The widening kernels stride
over rows beyond WIDEN_MAX_BLOCKS = 2048 blocks. A helper, not a test."""
import numpy as np

from paris_amd import backend as B

CAP_LANES = 4096 * 256
DIM_Y = 1030
BAND = (3, 1024)                      # rows 3 .. 1026
DIM_XS = (1025, 4100)                 # one pixel per lane; four pixels per lane (16-byte path)
GAP_ROWS = 3                          # rows of the buffer between frame 0 and frame 1
SENTINEL = np.uint32(0x7FC0BEEF)      # a NaN with a payload: whatever computes with it shows

WIDEN_ROWS = 4100                     # more than two visits of 2048 blocks
WIDEN_DIM_XS = (5, 8)                 # one pixel per lane; whole 16-byte vectors for every stored type


def lanes(dim_x, vector):
    return (dim_x // 4 if vector else dim_x) * BAND[1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Canvas:
    """Two frames of dim_x x DIM_Y in one pool buffer (rows padded to 256 bytes), GAP_ROWS rows apart, so the frame stride is larger
    than the frame. Everything around the frames -- the pitch padding and the gap -- holds SENTINEL. .first is frame 0 as a projection,
    .stride the bytes from one frame to the next."""

    def __init__(self, be, frames):
        assert len(frames) == 2
        self.be = be
        self.dim_y, self.dim_x = frames[0].shape
        self.rows = 2 * self.dim_y + GAP_ROWS
        self.owner = be.make_projection_device(self.dim_x, self.rows)
        self.pitch = self.owner.pitch
        self.width = self.pitch // 4
        assert self.pitch % 256 == 0 and self.width > self.dim_x, "a pool buffer with padded rows"
        self.stride = self.pitch * (self.dim_y + GAP_ROWS)
        self.first = be.wrap_projection(self.owner.ptr, self.pitch, self.dim_x, self.dim_y)
        self.all = B.Projection(self.owner.ptr, self.width, self.rows, pitch=self.pitch, on_device=True)
        self.before = np.full((self.rows, self.width), SENTINEL, np.uint32).view(np.float32)
        for k, f in enumerate(frames):
            self.frame_of(self.before, k)[:] = f
        self.write(self.before)

    def frame_of(self, canvas, k):
        first = k * (self.dim_y + GAP_ROWS)
        return canvas[first:first + self.dim_y, :self.dim_x]

    def write(self, canvas):
        self.be.copy_h2d(B.Projection(np.ascontiguousarray(canvas, np.float32), self.width, self.rows), self.all)

    def read(self):
        h = self.be.make_projection_host(self.width, self.rows)
        self.be.copy_d2h(self.all, h)
        return h.buf

    def expected(self, band_of_frame):
        """the canvas as it was, with rows BAND of frame k replaced by band_of_frame[k]"""
        want = self.before.copy()
        for k, band in enumerate(band_of_frame):
            self.frame_of(want, k)[BAND[0]:BAND[0] + BAND[1]] = band
        return want

    def free(self):
        self.be.free(self.owner)


def band_mask(canvas):
    """True on the pixels of both bands"""
    m = np.zeros((canvas.rows, canvas.width), bool)
    for k in range(2):
        canvas.frame_of(m, k)[BAND[0]:BAND[0] + BAND[1]] = True
    return m


def assert_canvas(canvas, got, want, what=""):
    """Inside the bands every pixel equals the rule's bit for bit, except that a NaN may carry any payload (which one a NaN that went
    through an operation carries is not part of the rules). Rows 0 .. 2 and 1027 .. 1029 of both frames, the pitch padding and the gap
    between the frames keep every bit, the sentinel's payload included."""
    inside = band_mask(canvas)
    assert np.array_equal(bits(got)[~inside], bits(canvas.before)[~inside]), (what, "outside the bands")
    g, w = got[inside], want[inside]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(w)[~nan]), (what, "the bands")
    return inside


def second_visit(canvas, a, k=0):
    """the pixels of frame k of canvas array `a` that the lanes past the cap serve: the last 1024 lanes of the band, which end its
    final row (1024 pixels, or 1024 groups of four)"""
    per_lane = 4 if canvas.dim_x % 4 == 0 else 1
    n = (lanes(canvas.dim_x, per_lane == 4) - CAP_LANES) * per_lane
    assert 0 < n <= canvas.dim_x
    return canvas.frame_of(a, k)[BAND[0] + BAND[1] - 1, canvas.dim_x - n:]
