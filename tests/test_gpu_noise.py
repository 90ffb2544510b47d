"""The native noise (`--rng native`) against oracle/philox_ref.py, the numpy statement of Philox4x32-10 + Box-Muller in the layout
include/vibo_hip.h documents, and every native trainer's draws against the schedule that header documents.

1. vibo_fill_normal entry by entry, at a counter word of the test's own: seeds with both key words set, steps up to 2^31 - 1,
   streams up to 2^32 - 1, lengths with every tail, views that start 4 / 8 / 12 bytes past a 16-byte boundary, and the counters
   whose radius uniform sits on either end of its 24-bit range.
2. what FusedTrainer, FusedCondFlowTrainer, FusedMeanTrainer and FusedDecoderTrainer consume with rng='native': step k (k completed
   steps) reads item noise from stream 0 and ability noise from stream 1 + rank, both at counter k.  The native trainer N runs
   beside a twin G of the same class that is handed what the test itself drew with vibo_fill_normal for that step; losses and
   parameters stay bit for bit the same, and where N's draws reach memory they are the test's fills."""
import functools

import numpy as np
import pytest
import torch

from gpu_common import assert_same_parameters, dev, fill_normal, noise_counter, record, simulated, twin_trainers
from oracle import philox_ref as P
from vibo_amd import decoder, ops
from vibo_amd.torch_core.models import VIBO_2PL
from vibo_amd.trainer import FusedCondFlowTrainer, FusedDecoderTrainer, FusedMeanTrainer, FusedTrainer

pytestmark = pytest.mark.gpu

BEEF = (0xDEADBEEF << 32) | 5
MAX64 = (1 << 64) - 1
STEP_MAX, STREAM_MAX = (1 << 31) - 1, (1 << 32) - 1
Q_BOUND = 4.0          # |z - z64| <= 4 q: see test_fill_normal_against_the_reference
SENTINEL = -1.25e30


# ---------------------------------------------------------------------------
# 1. vibo_fill_normal against the reference
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(n, seed, step, stream_id):
    """(z64, r, u, q) of the stream's first n entries: computed once per stream, shared, never written to."""
    z, r, u = P.normals(n, seed, step, stream_id)
    out = (z, r, u, P.resolution(r, u))
    for a in out:
        a.setflags(write=False)
    return out


def guarded_fill(n, seed, step, stream_id, offset=0):
    """vibo_fill_normal into a view that starts `offset` floats past a 16-byte boundary of a sentinel-filled buffer -> the n
    entries (host, float32); the elements on either side of the view have to keep their sentinel."""
    buf = torch.full((n + 12,), SENTINEL, device=dev())
    assert buf.data_ptr() % 16 == 0
    lo = 4 + offset
    fill_normal(n, seed, noise_counter(step), stream_id, out=buf[lo:lo + n])
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:lo] == SENTINEL).all()) and bool((host[lo + n:] == SENTINEL).all()), 'a guard element was written'
    return host[lo:lo + n].numpy()


def ratio_to_resolution(z, n, seed, step, stream_id):
    """max |z - z64| / q over the entries with r > 0; the entries with r = 0 (u = 1) have to be exact zeros, all have to be finite."""
    z64, r, u, q = reference(n, seed, step, stream_id)
    assert np.isfinite(z).all()
    zero = r == 0
    assert (z[zero] == 0).all()
    if zero.all():
        return 0.0
    return float((np.abs(z.astype(np.float64) - z64)[~zero] / q[~zero]).max())


# every seed {0, 7, both key words non-zero and distinct, all ones}, step {0, 1, 2^31 - 1}, stream {0, 1, 5, 2^32 - 1} and length
# appears; every length appears with a non-zero high seed word
FILL_CASES = [(1, MAX64, 0, 0), (3, BEEF, 1, 1), (4, MAX64, STEP_MAX, 5), (5, BEEF, 0, STREAM_MAX), (4099, MAX64, 1, 5),
              ((1 << 16) + 3, BEEF, STEP_MAX, 1), ((1 << 20) + 3, MAX64, STEP_MAX, STREAM_MAX), ((1 << 20) + 3, BEEF, 1, 0),
              (4099, 0, 0, 1), ((1 << 16) + 3, 7, 1, 5), ((1 << 20) + 3, 7, 0, 0), ((1 << 16) + 3, 0, STEP_MAX, STREAM_MAX)]


@pytest.mark.parametrize('n,seed,step,stream_id', FILL_CASES)
def test_fill_normal_against_the_reference(n, seed, step, stream_id):
    """Every entry within 4 q of the float64 reference, q = 2 pi r 2^-24 + 2^-24 / (u r) being what one step of either 24-bit
    uniform moves the entry by (the generator's own resolution; the same transform in numpy float32 is within 0.91 q).  A fault in
    the integer path -- round function, key schedule, a counter or key word -- moves an entry by O(1), about 10^6 q.  The margin
    over 0.91 is for v_log_f32, v_sin_f32, v_cos_f32 and sqrtf.  Measured on the MI355X over these cases: max |z - z64| / q = 0.45
    (2^20 + 3 entries of seed 7, step 0, stream 0; 0.44 at the all-ones seed and at 0xDEADBEEF00000005) -- below numpy's float32,
    whose angle 2 pi u is rounded once more before cos / sin while v_sin_f32 / v_cos_f32 take u in revolutions."""
    z = guarded_fill(n, seed, step, stream_id)
    worst = ratio_to_resolution(z, n, seed, step, stream_id)
    print('max |z - z64| / q', worst)
    record('fill_normal |z - z64| / q', worst, Q_BOUND, n=n, seed=seed, step=step, stream_id=stream_id)
    assert worst <= Q_BOUND


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_fill_normal_into_unaligned_views(offset):
    """A view 4, 8 or 12 bytes past a 16-byte boundary takes the one-float store path for every group: n = 0 ... 3 mod 4, below
    and above one workgroup's 1024 entries -- bit for bit the aligned fill, the guard elements on both sides untouched."""
    for n in (1, 2, 3, 4, 1027, 4097, 4098, 4099, 4100):
        aligned = guarded_fill(n, BEEF, 2, 5)
        shifted = guarded_fill(n, BEEF, 2, 5, offset=offset)
        assert np.array_equal(aligned.view(np.int32), shifted.view(np.int32)), n
        assert ratio_to_resolution(aligned, n, BEEF, 2, 5) <= Q_BOUND


# (step, group, word, 24-bit value) of seed BEEF, stream 0: found with the reference on the CPU over steps 0 ... 2^14 x groups
# 0 ... 2^14 (2^28 counters, 78 hits) -- the radius uniform c0 >> 8 (word 0: entries 4 g, 4 g + 1) or c2 >> 8 (word 2: entries
# 4 g + 2, 4 g + 3) is 0, the largest radius sqrt(48 ln 2) = 5.768, or 2^24 - 1, u = 1 and the radius 0
EXTREMES = [(2675, 614, 2, 0), (1866, 1550, 0, 0), (15577, 964, 2, 0), (3361, 2057, 0, 0),
            (16267, 635, 0, (1 << 24) - 1), (8791, 1953, 0, (1 << 24) - 1), (1067, 2512, 2, (1 << 24) - 1), (10246, 2709, 2, (1 << 24) - 1)]


@pytest.mark.parametrize('step,group,word,value', EXTREMES)
def test_fill_normal_at_the_ends_of_the_radius_uniform(step, group, word, value):
    """The stream up to and with the group whose radius uniform is extreme.  u = 1 (value 2^24 - 1): log2 gives 0, the radius 0, the
    pair has to be exact zeros.  u = 2^-24 (value 0): the reference's r and u are checked to be the ends; the kernel's pair is held
    through the 4 q bound only, which is loose there by its own definition -- q = 2 pi r 2^-24 + 2^-24 / (u r) is about 1 / r = 0.17
    at the smallest u, where one step of the uniform halves or doubles it -- but still excludes a non-finite or O(1)-wrong entry."""
    n = 4 * group + 4
    z64, r, u, q = reference(n, BEEF, step, 0)
    pair = slice(4 * group + word, 4 * group + word + 2)
    c = P.words(np.array([group], dtype=np.uint64), BEEF, step, 0)
    assert int(c[word][0]) >> 8 == value                     # (the hard-coded counter is what the scan found)
    z = guarded_fill(n, BEEF, step, 0)
    if value == 0:
        assert (u[pair] == 2.0 ** -24).all() and abs(r[pair][0] - np.sqrt(48 * np.log(2.0))) < 1e-12
    else:
        assert (u[pair] == 1.0).all() and (r[pair] == 0).all()
        assert (z[pair] == 0).all()
    assert ratio_to_resolution(z, n, BEEF, step, 0) <= Q_BOUND


# ---------------------------------------------------------------------------
# 2. what the native trainers consume
# ---------------------------------------------------------------------------
SEED = (0x5EED0BAD << 32) | 0x2468ACE1          # the trainers' seed: both key words non-zero and distinct
COND = dict(conditional_posterior=True)
FLOWS = dict(n_norm_flows=2)
DEEP = dict(generative_model='deep', hidden_dim=16)

# name: (trainer class, A, I, persons of the four steps, model keywords, trainer keywords, {persons: the planner's kernel})
CASES = {
    # the folded step: the matrix kernel draws its ability noise in the kernel; the shorter third minibatch runs on the VALU kernel
    'folded-matrix': (FusedTrainer, 8, 1000, (5000, 5000, 77, 5000), {}, {}, {5000: 'matrix', 77: 'VALU'}),
    'folded-valu': (FusedTrainer, 1, 1000, (300,) * 4, {}, {}, {300: 'VALU'}),
    'folded-narrow': (FusedTrainer, 2, 95, (77,) * 4, {}, {}, {77: 'narrow'}),
    # the four-launch form, whose prologue draws (vibo_train_prologue_noise)
    'unfolded-valu': (FusedTrainer, 1, 1000, (300,) * 4, {}, dict(fold=False), {300: 'VALU'}),
    'cond': (FusedCondFlowTrainer, 2, 200, (130,) * 4, COND, {}, {130: 'VALU'}),
    'flows': (FusedCondFlowTrainer, 2, 200, (130,) * 4, FLOWS, {}, {130: 'VALU'}),
    'cond-flows': (FusedCondFlowTrainer, 2, 200, (130,) * 4, {**COND, **FLOWS}, {}, {130: 'VALU'}),
    'mean': (FusedMeanTrainer, 2, 95, (77,) * 4, dict(ability_merge='mean'), {}, {77: 'VALU'}),
    # decoder.PERSON_CHUNK is patched to 64: 70 persons run as two chunks
    'deep': (FusedDecoderTrainer, 2, 60, (70,) * 4, DEEP, {}, {}),
    'deep-cond': (FusedDecoderTrainer, 2, 60, (70,) * 4, {**DEEP, **COND}, dict(conditional=True), {}),
}


def schedule_fills(I, D, B, A, k, ab_stream):
    """What the schedule says step k reads, drawn by the test into buffers of its own at a counter word of its own."""
    counter = noise_counter(k)
    return fill_normal(I * D, SEED, counter, 0).view(I, D), fill_normal(B * A, SEED, counter, ab_stream).view(B, A)


# The two words of a trainer's `_steps` are [Adam's step, completed steps], and the noise counter is the second.  They are equal
# between steps unless somebody makes them differ, and a drawing site that read the first would then go unnoticed whenever it
# reads before the same launch ticks it.  So N and G start with Adam's step ADAM_AHEAD steps ahead (the same bias correction in
# both twins, the noise counter still k): a site that reads word 0 draws at k + ADAM_AHEAD or k + ADAM_AHEAD + 1, never at k.
# The folded step is the documented exception (include/vibo_hip.h, vibo_train_epilogue_fused): its first launch ticks word 0 and
# its epilogue draws the NEXT step's head at counter step_count[0], which is completed steps + 1 only while the words move
# together -- the trainer refuses a second forward_backward() before update() for that reason.  Its words stay as they are.
ADAM_AHEAD = 3


def folded(tr):
    return type(tr) is FusedTrainer and tr.fold


def written_draws(tN, k, B, A, draws_in_kernel):
    """[(what, N's buffer, the step whose counter it was drawn at)] after N's step k, where the native path leaves its draws in
    memory.  The siblings' prologues write the noise of the step they start; the folded step's epilogue leaves the NEXT step's
    head behind (item noise always, the ability-noise buffer's whole capacity until a step has drawn in the kernel; after that a
    step on another kernel fills its own prefix in front of its launch, and a drawing step writes no ability noise at all)."""
    if not folded(tN):
        return [('item', tN._eps_item, k), ('ability', tN._eps_ab[B], k)]
    out = [('item', tN._eps_item, k + 1)]
    if not tN._draw_mode:
        out.append(('ability', tN._eps_cap, k + 1))
    elif not draws_in_kernel:
        out.append(('ability', tN._eps_cap[:B * A], k))
    return out


def follow_the_schedule(name, monkeypatch, rank=0, graph=False):
    """Four steps of N (rng='native') beside G (the test's fills handed in) -> the item noise N left in memory after every step.
    graph=True: the first step runs eagerly, then N's step is captured once and replayed three times against G's eager steps."""
    cls, A, I, persons, model_kw, trainer_kw, kernels = CASES[name]
    if graph:
        persons = persons[:1] * 4
    monkeypatch.setattr(decoder, 'PERSON_CHUNK', 64)
    d = dev()
    P_all = max(persons)
    resp, mask, _ = simulated(2, P_all, I, A, 0.1, seed=3)
    resp, mask = ops.pad_rows(resp.to(d), mask.bool().to(d))
    mN, mG, tN, tG = twin_trainers(VIBO_2PL, A, I, 5, dict(rng='native', seed=SEED, **trainer_kw), dict(trainer_kw), **model_kw)
    assert type(tN) is cls and type(tG) is cls
    mN._shard_rank = mG._shard_rank = rank          # (what enable_person_sharding sets; no reducer: one process, no group)
    ab_stream = 1 if cls is FusedDecoderTrainer else 1 + rank      # (the decoder step refuses person sharding and always draws stream 1)
    ahead = 0 if folded(tN) else ADAM_AHEAD
    for tr in (tN, tG):
        tr._steps[0] += ahead
    for B, kernel in kernels.items():
        assert ops.plan_kernel(mN.spec, B, I).startswith(kernel), (B, ops.plan_kernel(mN.spec, B, I))
    D = tN.item_mu.shape[1]
    captured, loss_g, seen_item, before = None, None, [], {}
    for k, B in enumerate(persons):
        rows = None if B == P_all else torch.arange(P_all - B, P_all, device=d)
        eps_item, eps_ab = schedule_fills(I, D, B, A, k, ab_stream)
        if graph and k == 1:
            torch.cuda.synchronize()
            captured = torch.cuda.CUDAGraph()
            with torch.cuda.graph(captured):
                loss_g = tN.step(resp, mask)                # capture only: nothing runs
        if captured is not None:
            captured.replay()
            lN = loss_g.clone()
        else:
            lN = tN.step(resp, mask, row_index=rows).clone()
        lG = tG.step(resp, mask, row_index=rows, eps_item=eps_item, eps_ability=eps_ab).clone()
        assert torch.equal(lN, lG) and bool(torch.isfinite(lN)), (k, float(lN), float(lG))
        assert_same_parameters(mN, mG)
        in_kernel = kernels.get(B) == 'matrix'
        if in_kernel:
            assert tN._draw_mode and tN.last.ability_mu is None      # (the drawing call leaves the posterior unwritten)
        for what, buf, at in written_draws(tN, k, B, A, in_kernel):
            stream_id = 0 if what == 'item' else ab_stream
            want = fill_normal(buf.numel(), SEED, noise_counter(at), stream_id)
            assert torch.equal(buf.reshape(-1).view(torch.int32), want.view(torch.int32)), (k, what)
            if what in before and before[what].numel() == buf.numel():
                assert not torch.equal(before[what], buf.reshape(-1)), (k, what, 'the draw of the step before')
            before[what] = buf.reshape(-1).clone()
        assert not torch.equal(eps_item, schedule_fills(I, D, B, A, k + 1, ab_stream)[0])
        seen_item.append(tN._eps_item.clone())
    assert tN._steps.tolist() == tG._steps.tolist() == [4 + ahead, 4]
    return seen_item


@pytest.mark.parametrize('name', list(CASES))
def test_native_trainer_consumes_the_documented_streams(name, monkeypatch):
    """Step k reads stream 0 (items) and stream 1 (abilities) of the trainer's seed at counter k: loss and every parameter of N
    equal G's bit for bit after each of four steps, N's noise buffers are the test's fills, and they change from step to step."""
    follow_the_schedule(name, monkeypatch)


@pytest.mark.parametrize('name', ['folded-matrix', 'cond-flows', 'mean', 'deep-cond'])
def test_native_trainer_replayed_from_a_graph_consumes_the_documented_streams(name, monkeypatch):
    """One case per trainer class: N's step captured once and replayed three times (the counters live on the device) against G
    stepping eagerly on the test's fills of counters 1, 2, 3."""
    follow_the_schedule(name, monkeypatch, graph=True)


@pytest.mark.parametrize('name', ['folded-matrix', 'folded-valu', 'unfolded-valu', 'cond-flows', 'mean', 'deep'])
def test_ranks_share_the_item_stream_and_own_their_ability_stream(name, monkeypatch):
    """Trainers on models whose _shard_rank is 0 and 3, in one process: the same item noise (stream 0 on every rank), ability noise
    from streams 1 and 4 -- read from memory where it is written, and through G on stream 4's fills where the matrix kernel draws
    it.  FusedDecoderTrainer refuses person sharding (a reducer) and passes stream 1 whatever the model's rank says: on a model
    with _shard_rank 3 it still draws stream 1."""
    rank0 = follow_the_schedule(name, monkeypatch, rank=0)
    rank3 = follow_the_schedule(name, monkeypatch, rank=3)
    for k, (a, b) in enumerate(zip(rank0, rank3)):
        assert torch.equal(a, b), k
