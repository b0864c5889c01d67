"""The dynamic LDS of the kernels that walk a tile of 16 trials over the learned flow (`fixed_points`, `smooth`, `sample_posterior`,
`ekf`), added up from the layouts of DESIGN.md section 3, in floats: what tests/test_fixed_point_host.py, test_smoother_host.py,
test_sampler_host.py, test_ekf_host.py and test_shape_range_ref.py hold the planners' answers against.

vg: columns of A per pass;  cl: centroids and w_mean in LDS;  sc: members per workgroup;  dl: the decoder in LDS.  LD = 17 floats per
feature row (16 trials and one of padding); a workgroup's budget is 159 KiB."""
BUDGET = 159 * 1024


def _common(n, d, dout, vg, cl, vectors, triangles):
    """The x step's buffers, 1 / width^2, `vectors` vectors, the dout x dout block, `triangles` lower triangles (given in halves:
    dout (dout + 1) / 2 each), one pass's partial products and (cl) the centroids and w_mean."""
    doutp = (dout + 15) // 16 * 16
    return (17 * (n + d + 4 * doutp + vectors * dout + dout * dout + triangles * dout * (dout + 1) // 2 + 4 * vg * doutp) + 2 * n
            + (n * d + n * dout if cl else 0))


def fixed_points(n, d, dout, vg, cl):
    return _common(n, d, dout, vg, cl, 3, 1)


def smooth(n, d, dout, vg, cl):
    return _common(n, d, dout, vg, cl, 4, 2)


def sample(n, d, dout, vg, sc, cl):
    return _common(n, d, dout, vg, cl, 2, 1) + 2 * sc * 2 * ((9 * dout) | 1)


def ekf(n, d, dout, dy, vg, cl, dl):
    dyp = (dy + 15) // 16 * 16
    ldc, ldt = (dy + 31) // 32 * 32 + 16, 16 if dout <= 16 else 48
    return _common(n, d, dout, vg, cl, 3, 3) + 17 * (16 + 1) + dout * dout + (dout * ldc + dyp * ldt if dl else 0)


def forms(lds, dout, floats, flags=1):
    """Every (vg, flag, ...) with 4 * floats(vg, flag, ...) == lds: what a plan's `lds` says of the form it took.  `floats(vg, *flags)`
    is one of the sums above with the shape filled in; `flags` is how many booleans follow vg."""
    out = []
    for vg in range(1, dout + 1):
        for bits in range(1 << flags):
            f = tuple(bool(bits >> i & 1) for i in range(flags))
            if 4 * floats(vg, *f) == lds:
                out.append((vg,) + f)
    return out
