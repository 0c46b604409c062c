"""The glue kernels of csrc/elementwise.hip in the modes the pipeline uses them in (sharded snippet
refine, periodic noise broadcast, per-frame depth gather, strided / repeated NCHW sources, vector-loop
and all-scalar min/max, strided transposes) — bitwise against plain PyTorch — and the attention
kernels' edges (small-KV context lengths 1..16 shared or per batch; Sq ≠ Sk with an explicit scale and
a strided output)."""
import pytest
import torch

from tests.test_kernels_gpu import attn_engine  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
DTYPES = [torch.float16, torch.float32]


def _k():
    from rollingdepth_amd import kernels as K
    return K


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ----------------------------------------------------------------------------- snippet refine
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("dil", [1, 2, 5])
def test_snippet_average_and_sharded_refine(dil, extra, dtype):
    """snippet_average against f64 per-frame sums ÷ cover count (f64 → f32 → dtype, bitwise); frames past
    the last snippet (extra = 2) and the padding channels come out as zeros.  The sharded form —
    snippet_accumulate over the shards (0, 3), (3, 0), (3, 4) of the snippets, summed, snippet_finish —
    gives the same bits, and its summed f64 partials are exactly the reference sums."""
    K_ = _k()
    n, w, h, wd, ld, c = 7, 3, 5, 7, 8, 4
    N = n + 2 * dil + extra
    g = torch.Generator().manual_seed(50 + dil)
    src = torch.randn(n, w, h, wd, ld, generator=g).to(dtype)  # padding channels hold junk, never read
    sums = torch.zeros(N, h, wd, c, dtype=torch.float64)
    cnt = torch.zeros(N, dtype=torch.float64)
    for s in range(n):
        for j in range(w):
            sums[s + j * dil] += src[s, j, ..., :c].double()
            cnt[s + j * dil] += 1
    assert (cnt[n + 2 * dil:] == 0).all() and (cnt[:n + 2 * dil] > 0).all()
    mean = torch.where(cnt.view(N, 1, 1, 1) > 0, sums / cnt.clamp_min(1).view(N, 1, 1, 1), torch.zeros(()).double())
    ref = mean.float().to(dtype)
    sd = src.to(DEV)
    avg = K_.snippet_average(sd, dil, N)
    assert avg.shape == (N, h, wd, ld) and avg.dtype == dtype
    assert torch.equal(_bits(avg[..., :c].cpu()), _bits(ref))
    assert (avg[..., c:] == 0).all() and (avg[n + 2 * dil:] == 0).all()
    total = sum(K_.snippet_accumulate(sd[k0:k0 + nloc], k0, dil, N) for k0, nloc in ((0, 3), (3, 0), (3, 4)))
    assert total.dtype == torch.float64 and torch.equal(total.cpu(), sums.view(N, h * wd, c))
    fin = K_.snippet_finish(total, n, w, dil, (h, wd), ld, dtype=dtype)
    assert torch.equal(_bits(fin), _bits(avg))


# ----------------------------------------------------------------------------- ddim_combine
def _ddim_check(y, x, e, ca, cb, s, c):
    """y[..., :c] within 1 ulp (of y's dtype) of (ca·x + cb·e)·s evaluated in f32 — as written, or with
    either product contracted into a fused multiply-add (the compiler's choice; where the two terms
    cancel the forms differ by more than an ulp of the result, so each is a candidate) — and zero
    padding.  f32 products and sums of two are exact in f64: the candidates are emulated there."""
    f32 = torch.float32
    ca_, cb_, s_ = (torch.tensor(v, dtype=f32).double().item() for v in (ca, cb, s))
    xd, ed = x.float().double(), e.float().double()
    px, pe = ca_ * xd, cb_ * ed  # exact
    cands = [(px.float().double() + pe.float().double()).float(), (px + pe.float().double()).float(),
             (px.float().double() + pe).float()]
    yd = y[..., :c].float().double()
    err = None
    for t in cands:
        r = (t.double() * s_).float().to(y.dtype)
        ex = torch.frexp(r.float().abs())[1].clamp_min(-13 if y.dtype == torch.float16 else -125)  # |r| < 2^ex
        ulp = torch.exp2((ex - (11 if y.dtype == torch.float16 else 24)).double())
        d = (yd - r.float().double()).abs() / ulp
        err = d if err is None else torch.minimum(err, d)
    print(f"ddim_combine {y.dtype}: max {err.max().item():.2f} ulp from the nearest evaluation order")
    assert err.max().item() <= 1.0
    assert (y[..., c:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_ddim_combine_periodic_noise(dtype):
    """One noise frame against five sample frames (e_period = 42 pixel rows), both channel slices of
    8-wide buffers."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(60)
    x = torch.randn(5, 6, 7, 8, device=DEV, generator=g).to(dtype)[..., :4]
    e = torch.randn(1, 6, 7, 8, device=DEV, generator=g).to(dtype)[..., :4]
    y = K_.ddim_combine(x, e, 0.3, -0.7, 2.0, 4, 8)
    assert y.shape == (5, 6, 7, 8) and y.dtype == dtype
    _ddim_check(y, x, e.expand(5, -1, -1, -1), 0.3, -0.7, 2.0, 4)
    with pytest.raises(ValueError):
        K_.ddim_combine(x, torch.randn(4, 6, 7, 8, device=DEV).to(dtype)[..., :4], 0.3, -0.7, 2.0, 4, 8)


def test_ddim_combine_grid_stride_second_trip():
    """P·Cpad = 16384·256 + 1000 elements: the grid (capped at 16384 blocks) takes a second trip."""
    K_ = _k()
    P = (16384 * 256 + 1000) // 8
    g = torch.Generator(device=DEV).manual_seed(61)
    x = torch.randn(P, 8, device=DEV, generator=g).half()[:, :4]
    e = torch.randn(P, 8, device=DEV, generator=g).half()[:, :4]
    y = K_.ddim_combine(x, e, 1.1, -0.4, 0.5, 4, 8)
    _ddim_check(y, x, e, 1.1, -0.4, 0.5, 4)


# ----------------------------------------------------------------------------- gather / layout
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_gather_unet_input_per_frame_depth(dtype):
    """depth_bcast=False (every refine step): depth frames gathered by the same indices as the rgb
    latents, with repeats; rgb a frame-strided view (every other frame of a larger buffer)."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(62)
    h, w = 5, 7
    big = torch.randn(10, h, w, 8, device=DEV, generator=g).to(dtype)
    rgb = big[::2]
    assert rgb.stride(0) == 2 * h * w * 8
    dep = torch.randn(5, h, w, 8, device=DEV, generator=g).to(dtype)
    idx = torch.tensor([4, 0, 4, 2, 1], dtype=torch.int32, device=DEV)
    u = K_.gather_unet_input(rgb, dep, idx, False)
    assert u.shape == (5, h, w, 8)
    assert torch.equal(u[..., :4], rgb[idx.long()][..., :4])
    assert torch.equal(u[..., 4:], dep[idx.long()][..., :4])


@pytest.mark.parametrize("src", ["repeat", "batch_strided"])
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("din,dout", [(torch.float32, torch.float16), (torch.float32, torch.float32),
                                      (torch.float16, torch.float16)], ids=["f32_f16", "f32_f32", "f16_f16"])
def test_nchw_to_nhwc_strided_sources(din, dout, C, src):
    """A stride-0 channel repeat (one channel expanded to C) and a batch-strided view (every other image),
    scaled by 0.5, to Cpad = 8: bitwise (x·scale) in f32 rounded once; the padding channels are zero."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(63)
    xbig = torch.randn(4, C, 5, 7, device=DEV, generator=g).to(din)
    x = xbig[:2, :1].expand(-1, C, -1, -1) if src == "repeat" else xbig[::2]
    assert x.stride(1) == (0 if src == "repeat" else 35) and not x.is_contiguous()
    y = K_.nchw_to_nhwc(x, 8, scale=0.5, dtype=dout)
    assert y.shape == (2, 5, 7, 8) and y.dtype == dout
    ref = (x.float() * 0.5).to(dout).permute(0, 2, 3, 1)
    assert torch.equal(_bits(y[..., :C]), _bits(ref))
    assert (y[..., C:] == 0).all()


# ----------------------------------------------------------------------------- minmax
_MM_THREADS = 2048 * 256  # minmax_partial's grid at these sizes
_MM_N = _MM_THREADS * 8 * 2 + 13


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["vector", "all_scalar"])
def test_minmax_vector_trips_and_scalar_paths(dtype, misaligned):
    """n = 2048·256·8·2 + 13: the 16-B vector loop runs two (f16) or four (f32) whole trips per thread and
    a ragged one, then the scalar tail.  The minimum sits at the last element (scalar tail), the maximum
    in the second trip of the vector loop (element 5 past one trip's reach: 2048·256 threads × 8 halves
    or 4 floats).  z[1:] is not 16-B aligned: every element goes through the scalar loop."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(64)
    z = torch.randn(_MM_N, device=DEV, generator=g).to(dtype)
    per = 8 if dtype == torch.float16 else 4
    imax = _MM_THREADS * per + 5
    assert _MM_N // per > imax // per >= _MM_THREADS and _MM_N % per  # a vector of the second trip; a scalar tail
    z[imax] = 9.5
    z[-1] = -9.25
    if misaligned:
        z = z[1:]
        assert z.data_ptr() % 16
    mm = K_.minmax(z)
    assert mm.dtype == torch.float32 and mm.tolist() == [-9.25, 9.5]
    # without the planted extremes: whatever the data's own are
    z[-1] = 0
    z[imax - (1 if misaligned else 0)] = 0
    mm = K_.minmax(z)
    assert mm[0].item() == z.min().item() and mm[1].item() == z.max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("n", [1, 7])
def test_minmax_tiny(n, dtype):
    """Fewer elements than one vector (f16) / fewer than two: most threads see nothing (±inf partials)."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(65)
    z = torch.randn(n, device=DEV, generator=g).to(dtype)
    mm = K_.minmax(z)
    assert mm[0].item() == z.min().item() and mm[1].item() == z.max().item()


# ----------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("rows,cols", [(1, 70), (64, 64), (65, 129), (130, 3)])
def test_transpose_strided(rows, cols, dtype):
    """Row-strided source (src_ld = cols + 3) into a wider, zero-filled destination (dst_ld = rows + 5)
    through out=: one row, exactly one 64×64 tile, one element past a tile in both directions, three
    columns.  The destination's padding stays zero."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(66)
    sbig = torch.randn(3, rows, cols + 3, device=DEV, generator=g).to(dtype)
    src = sbig[..., :cols]
    out = torch.zeros(3, cols, rows + 5, dtype=dtype, device=DEV)
    r = K_.transpose(src, out=out)
    assert r is out
    assert torch.equal(out[..., :rows], src.transpose(1, 2))
    assert (out[..., rows:] == 0).all()


def test_transpose_refuses_batch_strides_it_cannot_follow():
    """rdmi_transpose takes no batch stride (image b starts at b · rows · row stride): a row slice of a
    batched tensor, as source or destination, is refused instead of transposing the wrong rows; with
    one image the same view is fine."""
    K_ = _k()
    big = torch.randn(3, 40, 16, device=DEV).half()
    with pytest.raises(ValueError):
        K_.transpose(big[:, :33])
    with pytest.raises(ValueError):
        K_.transpose(big[:, :, :8].contiguous(), out=torch.zeros(3, 9, 40, dtype=torch.float16, device=DEV)[:, :8])
    with pytest.raises(ValueError):
        K_.transpose(big.transpose(1, 2))
    assert torch.equal(K_.transpose(big[:1, :33]), big[:1, :33].transpose(1, 2))


# ----------------------------------------------------------------------------- attention edges
def _sdpa_f64(q, k, v, heads, scale):
    B, Sq, HD = q.shape
    D = HD // heads
    qh = q.double().view(B, Sq, heads, D).transpose(1, 2)
    kh = k.double().view(B, -1, heads, D).transpose(1, 2)
    vh = v.double().view(B, -1, heads, D).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    return (p @ vh).transpose(1, 2).reshape(B, Sq, HD)


@pytest.mark.parametrize("per_batch", [False, True], ids=["shared_ctx", "per_batch_ctx"])
@pytest.mark.parametrize("L", [1, 7, 16])
def test_attention_smallkv_context_lengths(L, per_batch):
    """Every context length class the kernel takes (one key: softmax ≡ 1; odd; the maximum 16), the
    context shared ([1, L, C]) or one per batch element ([B, L, C]: kv batch stride), q a column slice
    of a fused [B, S, 3C] projection."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(70 + L)
    B, S, H = 2, 300, 5
    C = H * 64
    qkv = torch.randn(B, S, 3 * C, device=DEV, generator=g).half()
    q = qkv[..., C:2 * C]
    k = torch.randn(B if per_batch else 1, L, C, device=DEV, generator=g).half()
    v = torch.randn(B if per_batch else 1, L, C, device=DEV, generator=g).half()
    o = K_.attention_smallkv(q, k, v, H)
    ref = _sdpa_f64(q, k.expand(B, -1, -1), v.expand(B, -1, -1), H, 0.125)
    err = (o.double() - ref).abs().max().item()
    print(f"smallkv L={L} per_batch={per_batch}: max |d| {err:.2e}")
    assert err < 3e-3


def test_attention_smallkv_rejects_long_context():
    K_ = _k()
    q = torch.randn(1, 8, 64, device=DEV).half()
    kv = torch.randn(1, 17, 64, device=DEV).half()
    with pytest.raises(RuntimeError):
        K_.attention_smallkv(q, kv, kv, 1)


def test_attention_cross_lengths_scale_strided_out(attn_engine):
    """Sq = 100 against Sk = 333 keys (ragged last key tile), an explicit scale instead of 1/√d, and the
    output written into channels 64..64+C of a wider NaN-filled buffer, whose border stays NaN."""
    K_ = _k()
    g = torch.Generator(device=DEV).manual_seed(71)
    B, Sq, Sk, H = 2, 100, 333, 3
    C = H * 64
    q = torch.randn(B, Sq, C, device=DEV, generator=g).half()
    k = torch.randn(B, Sk, C, device=DEV, generator=g).half()
    v = torch.randn(B, Sk, C, device=DEV, generator=g).half()
    big = torch.full((B, Sq, C + 128), NAN, dtype=torch.float16, device=DEV)
    K_.attention(q, k, v, H, out=big[..., 64:64 + C], scale=0.2)
    ref = _sdpa_f64(q, k, v, H, 0.2)
    err = (big[..., 64:64 + C].double() - ref).abs().max().item()
    print(f"attention Sq={Sq} Sk={Sk} scale=0.2: max |d| {err:.2e}")
    assert err < 5e-3
    assert torch.isnan(big[..., :64]).all() and torch.isnan(big[..., 64 + C:]).all()
