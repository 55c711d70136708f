"""GPU parity of the HIP FFT / witness map / Groth16 prover (pcdhip_fft*, pcdhip_groth16_*; replace ark-poly
Radix2EvaluationDomain and ark-groth16 witness_map / create_proof reached from /root/reference
src/ec_cycle_pcd/mod.rs:171,179) against the CPU oracle and the golden vectors, through the C-ABI.
Bar: bit-exact (integer arithmetic)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_fft_golden(golden, gpu_ctx, fid):
    g = golden("fft")
    for log_n in (0, 1, 4, 8, 11):
        x = g[f"f{fid}_n{log_n}_in"]
        for inv in (0, 1):
            for coset in (0, 1):
                got = gpu_ctx.fft(fid, x, inverse=bool(inv), coset=bool(coset))
                assert np.array_equal(got, g[f"f{fid}_n{log_n}_i{inv}c{coset}"]), (fid, log_n, inv, coset)


@pytest.mark.parametrize("fid,logs", [(0, (2, 3, 5, 9, 10, 12, 13, 15, 16, 17)), (1, (6, 7, 10, 11, 14, 18)), (2, (5, 10, 11, 14, 15)), (3, (10, 12, 16))])
def test_fft_vs_oracle(co, gpu_ctx, fid, logs):
    for log_n in logs:
        x = co.gen_field(fid, 1 << log_n, seed=log_n)
        for inv in (False, True):
            for coset in (False, True):
                want = co.fft(fid, x, inverse=inv, coset=coset, nthreads=16)
                assert np.array_equal(gpu_ctx.fft(fid, x, inverse=inv, coset=coset), want), (fid, log_n, inv, coset)


@pytest.mark.parametrize("fid,q", [(0, 7), (2, 5)])
def test_mixed_radix_fft(co, gpu_ctx, fid, q):
    """K2m: MixedRadixEvaluationDomain transforms (the help-proof domains beyond 2^17 / 2^15) vs the oracle."""
    for m, a in ((q, 3), (q * q, 2), (q, 11), (q * q, 10), (q, 13)):
        n = m << a
        x = co.gen_field(fid, n, seed=n)
        for inv in (False, True):
            for coset in (False, True):
                want = co.fft_general(fid, x, m, inverse=inv, coset=coset, nthreads=16)
                assert np.array_equal(gpu_ctx.fft_general(fid, x, inverse=inv, coset=coset), want), (fid, m, a, inv, coset)
    from pcd_amd import capi
    with pytest.raises(capi.PcdHipError):
        gpu_ctx.fft_general(fid, np.zeros((3 * 64, x.shape[1]), dtype=np.uint64))  # 3 * 2^6 is not a domain size


def _structured_inputs(fid, n):
    """all zero, all p - 1, a delta at index 0 and at index n - 1, a constant c, alternating 0 / p - 1 (C-ABI Montgomery images);
    the butterflies of the other FFT tests only ever see random residues"""
    from oracle import pyoracle as O
    f = O.FIELDS[fid]
    c = (f.p - 1) // 3 + 5
    row = lambda v: O.pack_fp(f, [v])[0]
    zero, top, one, cst = row(0), row(f.p - 1), row(1), row(c)
    full = lambda r: np.ascontiguousarray(np.tile(r, (n, 1)))
    d0, dn, alt = full(zero), full(zero), full(zero)
    d0[0] = one
    dn[n - 1] = one
    alt[1::2] = top
    return {"zero": full(zero), "p-1": full(top), "delta0": d0, "delta_last": dn, "const": full(cst), "alt": alt}, c


# one log_n per kernel path (fft.hip.h): a single pass up to 10 -- 0 and 1 are the degenerate and the smallest transform (no twiddled layer);
# 9 and 10 are the sizes at which fft_pass_kernel renormalises the lazily reduced 298-bit elements (blog > 8 in the one-layer loop, blog > 7
# in the two-layer loop: unreduced values stack 8 - 9 layers deep only there, and 2^10 is the largest LDS tile) -- two passes from 11, three from 15
@pytest.mark.parametrize("log_n", [0, 1, 9, 10, 11, 15])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_fft_structured_vectors(co, gpu_ctx, fid, log_n):
    from oracle import pyoracle as O
    f = O.FIELDS[fid]
    n = 1 << log_n
    ins, c = _structured_inputs(fid, n)
    for name, x in ins.items():
        for inv in (False, True):
            for coset in (False, True):
                got = gpu_ctx.fft(fid, x, inverse=inv, coset=coset)
                assert np.array_equal(got, co.fft(fid, x, inverse=inv, coset=coset, nthreads=16)), (fid, log_n, name, inv, coset)
                if not inv and not coset and name == "delta0":     # closed forms, in Python integers: all ones
                    assert np.array_equal(got, np.tile(O.pack_fp(f, [1])[0], (n, 1))), (fid, log_n, name)
                if not inv and not coset and name == "const":      # n c at index 0, zero elsewhere
                    assert O.unpack_fp(f, got[:1])[0] == n * c % f.p and not got[1:].any(), (fid, log_n, name)


@pytest.mark.parametrize("fid,m", [(0, 7), (2, 5)])
def test_mixed_radix_fft_structured_vectors(co, gpu_ctx, fid, m):
    from oracle import pyoracle as O
    f = O.FIELDS[fid]
    n = m << 3
    ins, c = _structured_inputs(fid, n)
    for name, x in ins.items():
        for inv in (False, True):
            for coset in (False, True):
                got = gpu_ctx.fft_general(fid, x, inverse=inv, coset=coset)
                assert np.array_equal(got, co.fft_general(fid, x, m, inverse=inv, coset=coset, nthreads=16)), (fid, m, name, inv, coset)
                if not inv and not coset and name == "delta0":
                    assert np.array_equal(got, np.tile(O.pack_fp(f, [1])[0], (n, 1))), (fid, m, name)
                if not inv and not coset and name == "const":
                    assert O.unpack_fp(f, got[:1])[0] == n * c % f.p and not got[1:].any(), (fid, m, name)


@pytest.mark.parametrize("fid,n", [(1, 1 << 12), (3, 1 << 9), (0, 7 << 6), (2, 25 << 4)])
def test_fft_seq_one_round_trip(co, gpu_ctx, fid, n):
    """pcdhip_fft_seq (seam S2: a chain of transforms on one host vector, one trip over PCIe) == the same transforms one call at a time ==
    the oracle: the witness map's `ifft; coset_fft`, its inverse, and all four kinds in a row; radix-2 and mixed-radix domains"""
    x = co.gen_field(fid, n, seed=n + fid)
    m = n
    while m % 2 == 0:
        m //= 2
    ref = (lambda v, inv, cos: co.fft(fid, v, inverse=inv, coset=cos, nthreads=8)) if m == 1 else \
          (lambda v, inv, cos: co.fft_general(fid, v, m, inverse=inv, coset=cos, nthreads=8))
    for ops in ([(True, False), (False, True)], [(True, True), (False, False)], [(False, False), (False, True), (True, True), (True, False)]):
        want = x
        for inv, cos in ops:
            want = ref(want, inv, cos)
        assert np.array_equal(gpu_ctx.fft_seq(fid, x, ops), want), (fid, n, ops)
    from pcd_amd import capi
    with pytest.raises(capi.PcdHipError):
        gpu_ctx.fft_seq(fid, np.zeros((3 * 64, x.shape[1]), dtype=np.uint64), [(False, False)])


@pytest.mark.parametrize("cid,nc", [(1, (1 << 17) + 1000), (3, (1 << 15) + 500)])
def test_witness_map_mixed_radix_domain(co, gpu_ctx, cid, nc):
    """help-proof witness map on a domain beyond the help field's 2-adicity (7 * 2^15 / 5 * 2^13 elements)."""
    fr = co.CURVE_FR[cid]
    r = co.synthetic_r1cs(fr, nc, 2, seed=nc)
    want = co.witness_map(r, nthreads=32)
    got = gpu_ctx.witness_map(fr, r)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_fft_size_limits(gpu_ctx):
    from pcd_amd import capi
    with pytest.raises(capi.PcdHipError):  # 2-adicity of F298A is 17: needs the mixed-radix domain
        gpu_ctx.fft(0, np.zeros((1 << 18, 5), dtype=np.uint64))


@pytest.mark.parametrize("fid,log_n", [(1, 20), (3, 20)])
def test_fft_full_size_roundtrip(co, gpu_ctx, fid, log_n):
    """BASELINE size 2^20: ifft(fft(x)) = x, coset variants, and linearity on device-resident vectors."""
    n = 1 << log_n
    x = co.gen_field(fid, n, seed=1)
    for coset in (False, True):
        xb = gpu_ctx.buf_upload(fid, x)
        gpu_ctx.fft(fid, xb, coset=coset)
        fx = xb.download()
        gpu_ctx.fft(fid, xb, inverse=True, coset=coset)
        assert np.array_equal(xb.download(), x)
        xb.free()
        # spot check of the forward transform against the oracle on a decimated problem is not possible;
        # compare the whole vector for the 298-bit field (the oracle needs ~1 s), linearity for 753
        if fid == 1:
            assert np.array_equal(fx, co.fft(fid, x, coset=coset, nthreads=32))
    y = co.gen_field(fid, n, seed=2)
    fy = gpu_ctx.fft(fid, y)
    fxy = gpu_ctx.fft(fid, co.fp_op(fid, "add", x, y))
    assert np.array_equal(fxy, co.fp_op(fid, "add", gpu_ctx.fft(fid, x), fy))


def _golden_r1cs(co, g, cid):
    pre = f"c{cid}_"
    return co.R1CS(co.CURVE_FR[cid], int(g[pre + "num_inputs"][0]), g[pre + "rp_a"], g[pre + "col_a"], g[pre + "coeff_a"],
                   g[pre + "rp_b"], g[pre + "col_b"], g[pre + "coeff_b"], g[pre + "rp_c"], g[pre + "col_c"],
                   g[pre + "coeff_c"], np.ascontiguousarray(g[pre + "z"]))


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_witness_map_golden(co, golden, gpu_ctx, cid):
    g = golden("groth16")
    r = _golden_r1cs(co, g, cid)
    assert np.array_equal(gpu_ctx.witness_map(co.CURVE_FR[cid], r), g[f"c{cid}_h"])


@pytest.mark.parametrize("cid,nc", [(0, 3000), (1, 1000), (0, (1 << 16) - 3), (2, 700), (3, 300)])
def test_witness_map_vs_oracle(co, gpu_ctx, cid, nc):
    fr = co.CURVE_FR[cid]
    r = co.synthetic_r1cs(fr, nc, 3, seed=nc)
    assert np.array_equal(gpu_ctx.witness_map(fr, r), co.witness_map(r, nthreads=16))


@pytest.mark.parametrize("cid,nc", [(0, 20000), (1, 9000), (2, 9000), (3, 9000), (0, 50)])
def test_witness_map_skewed_matrix(co, gpu_ctx, cid, nc):
    """the shape `cs.finalize()` leaves of a verifier circuit (coracle.skewed_r1cs: power-law row lengths with rows above 4096
    entries, >= 80 % unit coefficients, small integers, a few random ones): the mat-vec kernels take the small-integer entries through
    additions, the others through products, rows above 16 entries with a wave each -- h equal to the oracle's, through the call that
    hands the matrices over and through the resident-matrix path"""
    fr = co.CURVE_FR[cid]
    r = co.skewed_r1cs(fr, nc, 2, seed=300 + nc + cid)
    want = co.witness_map(r, nthreads=16)
    assert np.array_equal(gpu_ctx.witness_map(fr, r), want)
    keys = co.synthetic_keys(cid, r, seed=301)
    pk = gpu_ctx.g16_pk_upload(keys.host_struct(), cid)
    gpu_ctx.g16_pk_set_r1cs(pk, r)
    try:
        h, ms = gpu_ctx.witness_map_resident(pk, r)
        assert np.array_equal(h, want) and ms["total"] > 0
        rs = co.gen_field(fr, 2, seed=302)
        got, inf = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1], resident_r1cs=True)
        w, winf = co.groth16_prove(keys, r, rs[0], rs[1], nthreads=16)
        assert np.array_equal(got, w) and np.array_equal(inf, winf)
    finally:
        pk.free()


@pytest.mark.parametrize("cid,nc", [(0, 30000), (3, 6000)])
def test_prove_keys_with_points_at_infinity(co, gpu_ctx, cid, nc):
    """The a / b queries of a real key hold the point at infinity for every variable that no row of A / B mentions (a third of them in
    this R1CS).  Their entries are left out of the MSMs' bucket lists, and which MSMs of a proof share a sort depends on them
    (capi_g16_prove.hip G16Run::launch_assignment): the key as a setup makes it, the key with every entry finite, and a key whose b_g1 / b_g2 flags
    differ, each through both assembly forms -- the proof equal to the oracle's every time.  (Whatever coordinates a flagged entry holds
    are ignored: the synthetic key keeps its seeded points there.)"""
    fr = co.CURVE_FR[cid]
    r = co.skewed_r1cs(fr, nc, 2, seed=330 + cid)
    rs = co.gen_field(fr, 2, seed=331)
    variants = []
    sparse = co.synthetic_keys(cid, r, seed=332)
    assert 0.1 < sparse.a_inf.mean() < 0.6 and 0.2 < sparse.b_g2_inf.mean() < 0.7 and not sparse.a_inf[:r.num_inputs].any()
    variants.append(sparse)
    variants.append(co.synthetic_keys(cid, r, seed=332, consistent=False))
    odd = co.synthetic_keys(cid, r, seed=332)
    i = int(np.flatnonzero(odd.b_g1_inf)[3])
    odd.b_g1_inf[i] = 0                      # b_g1 finite where b_g2 is infinite: the two B MSMs may not share a list
    variants.append(odd)
    only_a = co.synthetic_keys(cid, r, seed=332); only_a.b_g1_inf[:] = 0; only_a.b_g2_inf[:] = 0    # (each combination shares sorts differently)
    only_b = co.synthetic_keys(cid, r, seed=332); only_b.a_inf[:] = 0
    variants += [only_a, only_b]
    for keys in variants:
        want, winf = co.groth16_prove(keys, r, rs[0], rs[1], nthreads=16)
        pk = gpu_ctx.g16_pk_upload(keys.host_struct(), cid)
        try:
            for mode in (1, 2, 0):
                gpu_ctx.groth16_set_assembly(mode)
                got, inf = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1])
                assert np.array_equal(got, want) and np.array_equal(inf, winf), (mode, float(keys.b_g2_inf.mean()))
        finally:
            gpu_ctx.groth16_set_assembly(0)
            pk.free()
    # a plain MSM over a vector with flagged entries, scalars of every kind on them (random, zero, one)
    n = 5000
    pts = co.gen_points(cid, 1, n, seed=333)
    inf = (np.arange(n) % 3 == 0).astype(np.uint8)
    sc = co.gen_scalars(fr, n, seed=334, dist=1)
    b = gpu_ctx.bases_upload(cid, 1, pts, inf=inf)
    sb = gpu_ctx.buf_upload(fr, sc)
    try:
        got = gpu_ctx.msm(b, sb)
    finally:
        b.free(); sb.free()
    assert np.array_equal(co.to_affine(cid, 1, got)[0], co.to_affine(cid, 1, co.msm(cid, 1, pts, sc, inf=inf, nthreads=8))[0])


@pytest.mark.parametrize("cid", [0, 1])
def test_groth16_golden_proof(co, golden, gpu_ctx, cid):
    """Keys and expected proof come from the pure-Python oracle (tests/golden/groth16.npz)."""
    g = golden("groth16")
    pre = f"c{cid}_"
    r = _golden_r1cs(co, g, cid)
    arrays = {k: np.ascontiguousarray(g[pre + k]) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "gamma_g2",
                                                            "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "gamma_abc_g1")}
    arrays.update(a_inf=g[pre + "a_query_inf"], b_g1_inf=g[pre + "b_g1_query_inf"], b_g2_inf=g[pre + "b_g2_query_inf"],
                  h_inf=g[pre + "h_query_inf"], l_inf=g[pre + "l_query_inf"], gamma_abc_inf=g[pre + "gamma_abc_g1_inf"])
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    keys = co.Keys(cid, r, arrays)
    for mode in (-1, 0):
        gpu_ctx.set_precompute(mode)
        pk = gpu_ctx.g16_pk_upload(keys.host_struct(), cid)
        proof, inf = gpu_ctx.groth16_prove(pk, r, g[pre + "r"], g[pre + "s"])
        pk.free()
        assert np.array_equal(proof, g[pre + "proof"]) and not inf.any()
    gpu_ctx.set_precompute(-1)


@pytest.mark.parametrize("cid,nc", [(0, 2000), (1, 1200), (2, 150), (3, 60)])
def test_groth16_roundtrip(co, gpu_ctx, cid, nc):
    """Mirror of tests/mnt4_groth16.rs:84-87,119 at the SNARK level, with the proof made by the HIP path:
    setup (oracle) -> prove (GPU) -> verify accepts; a wrong public input rejects; proof == oracle's proof."""
    fr = co.CURVE_FR[cid]
    r = co.synthetic_r1cs(fr, nc, 3, seed=100 + cid)
    keys = co.groth16_setup(cid, r, co.gen_field(fr, 5, seed=7), nthreads=32)
    rs = co.gen_field(fr, 2, seed=8)
    pk = gpu_ctx.g16_pk_upload(keys.host_struct(), cid)
    proof, inf = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1])
    gpu_ctx.g16_pk_set_r1cs(pk, r)
    proof2, inf2 = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1], resident_r1cs=True)
    gpu_ctx.groth16_set_assembly(1)  # s*A and r*B_1 as two more MSMs ...
    proof3, inf3 = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1], resident_r1cs=True)
    gpu_ctx.groth16_set_assembly(2)  # ... or as chained one-lane products (0, the default, picks one of the two)
    proof4, inf4 = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1], resident_r1cs=True)
    gpu_ctx.groth16_set_assembly(0)
    # the G1 accumulations as pair trees of affine additions (753-bit curves; the others ignore the mode): five MSM streams, the
    # shared sort of the assignment feeding tree kernels, chunks small enough that runs cross chunk edges
    gpu_ctx.msm_set_accumulate(2, 40, 2)
    try:
        proof5, inf5 = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1], resident_r1cs=True)
    finally:
        gpu_ctx.msm_set_accumulate(0)
    pk.free()
    want, winf = co.groth16_prove(keys, r, rs[0], rs[1], nthreads=16)
    assert np.array_equal(proof, want) and np.array_equal(inf, winf)
    assert np.array_equal(proof2, want) and np.array_equal(inf2, winf)
    assert np.array_equal(proof3, want) and np.array_equal(inf3, winf)
    assert np.array_equal(proof4, want) and np.array_equal(inf4, winf)
    assert np.array_equal(proof5, want) and np.array_equal(inf5, winf)
    pub = np.ascontiguousarray(r.z[1:r.num_inputs])
    assert co.groth16_verify(keys, pub, proof)
    bad = pub.copy()
    bad[1] = co.fp_op(fr, "add", bad[1:2], r.z[:1])[0]
    assert not co.groth16_verify(keys, bad, proof)


# ---- key generation: fixed-base batches and generate_parameters ------------------------------
FB_SIZES = [(0, 1, 300), (0, 2, 100), (1, 1, 300), (1, 2, 70), (2, 1, 40), (2, 2, 20), (3, 1, 40), (3, 2, 12)]
# fb_normalize_kernel shares one inversion among the 8 points of a lane: one lane short of a batch, exactly one, one with a lone point
# behind it, and a second workgroup that holds a single point (64 lanes x 8 + 1), on the smallest and on the largest group
FB_SIZES += [(cid, group, n) for cid, group in ((0, 1), (3, 2)) for n in (1, 7, 8, 9, 64 * 8 + 1)]


def _fb_zero_slots(n):
    """where the scalars are zero (the results infinite): slot 0, the middle and the last slot of the first batch of 8, the same of the
    second batch, the whole third batch, and the last point of all (alone in its batch for n = 9 and n = 64 * 8 + 1); the slots 1 .. 4
    keep their edge scalars"""
    z = {0}
    if n > 5:
        z |= {5, min(7, n - 1), n - 1}
    if n >= 16:
        z |= {11, 15}
    if n >= 24:
        z |= set(range(16, 24))
    return sorted(z)


@pytest.mark.parametrize("cid,group,n", FB_SIZES)
def test_fixed_base_mul_vs_oracle(co, gpu_ctx, cid, group, n):
    """FixedBaseMSM::multi_scalar_mul + batch normalisation: out[i] = k_i * G, affine -- EVERY output and flag against the oracle's
    fixed-base batch, a sample of them against its double-and-add as well; scalars include 0, 1, r - 1 and window-boundary values, and
    zeros (infinite results) at the start, in the middle and at the end of a batch of 8 and through a whole one."""
    fr = co.CURVE_FR[cid]
    sc = co.gen_scalars(fr, n, seed=40 + cid)
    one = np.zeros_like(sc[:1]); one[0, 0] = 1
    edge = [0, 1, 255, 256]
    for i, v in enumerate(edge[:n]):
        sc[i] = 0; sc[i, 0] = v
    if n > 4:
        sc[4] = co.fp_op(fr, "to_canonical", co.fp_op(fr, "neg", co.fp_op(fr, "from_canonical", one)))[0]   # r - 1
    zeros = _fb_zero_slots(n)
    sc[zeros] = 0
    assert sc[[i for i in range(n) if i not in zeros]].any(axis=1).all()
    base = co.generator(cid, group)
    got, inf = gpu_ctx.fixed_base_mul(cid, group, base, sc)
    want_all, winf_all = co.fixed_base_mul(cid, group, base, sc)
    assert np.array_equal(inf, winf_all) and list(np.flatnonzero(inf)) == zeros
    assert not got[inf != 0].any() and np.array_equal(got[inf == 0], want_all[inf == 0])
    # (the double-and-add takes 0.3 s per point on G2 of a 753-bit curve: two samples behind the first batch at the largest size)
    for i in list(range(min(8, n))) + (list(range(8, n, max(1, n // 24))) if n <= 300 else [n // 2, n - 2]):
        want, winf = co.to_affine(cid, group, co.scalar_mul(cid, group, base, sc[i])[None])
        assert inf[i] == winf[0] and (inf[i] or np.array_equal(got[i], want[0])), i
    assert inf[0] == 1 and not got[0].any() and (n < 2 or np.array_equal(got[1], base))
    # an infinity base and an empty batch
    z, zinf = gpu_ctx.fixed_base_mul(cid, group, np.zeros_like(base), sc[:9])
    assert zinf.all() and not z.any()
    e, einf = gpu_ctx.fixed_base_mul(cid, group, base, sc[:0])
    assert e.shape[0] == 0


@pytest.mark.parametrize("cid,nc", [(0, 700), (1, 500), (2, 90), (3, 40)])
def test_groth16_setup_vs_oracle(co, gpu_ctx, cid, nc):
    """generate_parameters on the device == the oracle's generator on the same toxic waste, every query bit-exact;
    the GPU-made key then proves (GPU) and verifies (oracle pairing), as tests/mnt4_groth16.rs:84-87 does end to end."""
    fr = co.CURVE_FR[cid]
    r = co.synthetic_r1cs(fr, nc, 3, seed=300 + cid)
    toxic = co.gen_field(fr, 5, seed=17)
    want = co.groth16_setup(cid, r, toxic, nthreads=32)
    K = gpu_ctx.groth16_setup(cid, r, co.generator(cid, 1), co.generator(cid, 2), toxic)
    for name in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2", "a_query", "a_inf", "b_g1_query", "b_g1_inf",
                 "b_g2_query", "b_g2_inf", "h_query", "h_inf", "l_query", "l_inf", "gamma_abc_g1", "gamma_abc_inf"):
        assert np.array_equal(K[name], getattr(want, name)), name
    keys = co.Keys(cid, r, {k: v for k, v in K.items() if k != "domain_size"})
    rs = co.gen_field(fr, 2, seed=18)
    pk = gpu_ctx.g16_pk_upload(keys.host_struct(), cid)
    proof, inf = gpu_ctx.groth16_prove(pk, r, rs[0], rs[1])
    pk.free()
    assert co.groth16_verify(keys, np.ascontiguousarray(r.z[1:r.num_inputs]), proof)


def test_groth16_setup_rejects_tau_in_domain(co, gpu_ctx):
    """tau = 1 is a domain element: upstream never samples it (sample_element_outside_domain); the library refuses."""
    from pcd_amd import capi
    fr = co.CURVE_FR[0]
    r = co.synthetic_r1cs(fr, 100, 2, seed=5)
    toxic = co.gen_field(fr, 5, seed=17)
    one = np.zeros_like(toxic[:1]); one[0, 0] = 1
    toxic[4] = co.fp_op(fr, "from_canonical", one)[0]
    with pytest.raises(capi.PcdHipError):
        gpu_ctx.groth16_setup(0, r, co.generator(0, 1), co.generator(0, 2), toxic)
