"""k_gru_h16r (the first GRU in two wave roles, rl4rs_amd/csrc/gru_roles.hpp; the default) against the 4-wave k_gru_h16 + k_h1_frag
(scorer_kernels='gru_h16_v1'), each with and without the pad table ('no_gru_pad'): the h1 cache, its fragment-order copy and lead[]
bit for bit, and h1 against the fp64 oracle at the bar tests/test_gpu_dien.py uses for the first GRU's cache (2e-6 abs).  Every
handle of one maxlen sees the same encodes in the same order, so a fragment row or a zero tail that one path leaves stale shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 3000
CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": H, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32, "scorer_precision": "fp16x2"}
VARIANTS = ['', 'gru_h16_v1', 'no_gru_pad', 'gru_h16_v1,no_gru_pad']
SLOTS = 80
H1_BAR = 2e-6                       # tests/test_gpu_dien.py::test_dien_rowwise_matches_oracle, first-GRU cache


def ids_of(pattern, cnt, L, rs):
    b = rs.randint(1, H, size=(cnt, L))
    b[0, L - 1] = 1
    b[cnt - 1, L - 1] = H - 1                                 # the table's last row
    if pattern == 'allzero':
        b[:] = 0
    elif pattern == 'common':                                 # 55 zeros in front of every row at maxlen 64
        b[:, :(55 * L) // 64] = 0
    elif pattern == 'mixed':                                  # t0 = 0 (row 0 has no prefix) while single rows have lead > 0
        for r in range(cnt):
            b[r, :(r * 5) % (L + 1)] = 0
    elif pattern == 'middle':                                 # zeros further in are ordinary steps on id 0
        b[:, :min(3, L - 1)] = 0
        b[:, L // 2:L // 2 + 5] = 0
        b[cnt // 2, min(3, L - 1)] = 0
    elif pattern == 'last':                                   # t0 = L - 1: one computed step
        b[:, :L - 1] = 0
    else:
        assert pattern == 'none'
    return np.ascontiguousarray(b.astype(np.int32))


def frag_of(h1):
    """h1 [slots, L, 128] -> the fragment order of din_x.hpp, steps L .. 32 NT - 1 zero"""
    n, L, _ = h1.shape
    NT = (L + 31) // 32
    p = np.zeros((n, NT * 32, 128), dtype=h1.dtype)
    p[:, :L] = h1
    # [slot][n][t % 32][kb][kg][8] -> [slot][n][kb][kg * 32 + t % 32][8]
    return p.reshape(n, NT, 32, 8, 2, 8).transpose(0, 1, 3, 4, 2, 5).reshape(n, NT, 8, 64, 8)


class Handles(object):
    def __init__(self, L):
        import torch
        from rl4rs_amd.nets.dien import init_dien_weights
        from rl4rs_amd.device import DeviceDien
        from oracle.dien import OracleDien
        self.torch, self.L = torch, L
        self.cfg = dict(CFG, maxlen=L)
        self.w = init_dien_weights(self.cfg, seed=8, emb_scale=0.5, bias_noise=0.2)
        self.nets = [DeviceDien(dict(self.cfg, scorer_kernels=k), self.w, max_rows=SLOTS, max_slots=SLOTS) for k in VARIANTS]
        self.orc = OracleDien(self.w, self.cfg, np.float64)
        self.want = np.zeros((SLOTS, L, 128))                 # fp64 states of what the slots hold
        self.lead = np.zeros(SLOTS, dtype=np.int64)
        self.live = np.zeros(SLOTS, dtype=bool)

    def encode(self, ids, slot_base):
        from rl4rs_amd.device import DIEN_H1, DIEN_H1_FRAG, DIEN_LEAD
        torch, cnt = self.torch, ids.shape[0]
        for net in self.nets:
            net.encode(0, torch.from_numpy(ids).cuda(), slot_base)
        self.want[slot_base:slot_base + cnt] = self.orc.gru(self.orc.w['seq_emb'][ids], 0)
        nz = ids != 0
        self.lead[slot_base:slot_base + cnt] = np.where(nz.any(1), nz.argmax(1), self.L)
        self.live[slot_base:slot_base + cnt] = True
        live = torch.from_numpy(self.live).cuda()
        h1 = [net.snapshot(DIEN_H1, SLOTS)[live] for net in self.nets]
        fr = [net.snapshot(DIEN_H1_FRAG, SLOTS)[:SLOTS][live] for net in self.nets]
        for k in range(1, 4):                                 # every slot ever written, not only this encode's
            assert torch.equal(h1[0], h1[k]), VARIANTS[k]
            assert torch.equal(fr[0], fr[k]), VARIANTS[k]
        assert np.array_equal(fr[0].cpu().numpy(), frag_of(h1[0].cpu().numpy()))
        assert np.abs(h1[0].cpu().numpy() - self.want[self.live]).max() < H1_BAR
        lead = [net.snapshot(DIEN_LEAD, SLOTS)[:SLOTS][live].cpu().numpy() for net in self.nets[:2]]
        assert np.array_equal(lead[0], lead[1]) and np.array_equal(lead[0], self.lead[self.live])
        # the all-zero sequence's slot behind max_slots, written when the handle was created
        pad = [net.snapshot(DIEN_H1_FRAG, SLOTS)[SLOTS] for net in self.nets[:2]]
        assert torch.equal(pad[0], pad[1])

    def close(self):
        for net in self.nets:
            net.close()


@pytest.fixture(scope='module', params=[1, 2, 33, 64])
def hs(request):
    h = Handles(request.param)
    yield h
    h.close()


def test_labels_name_the_kernel_that_runs(hs):
    import ctypes as C
    from rl4rs_amd import _lib
    assert 'gru_h16_v1' in _lib.DIEN_OPTS
    names = []
    for net in hs.nets[:2]:
        labels = []
        for k in range(net.lib.rl4rs_dien_kernel_count()):
            buf = C.create_string_buffer(160)
            assert net.lib.rl4rs_dien_kernel_label(net.h, k, buf, 160) == 0
            labels.append(buf.value.decode())
        names.append([x for x in labels if 'gru_h16' in x])
    assert names[0] == ['k_gru_h16r'] and names[1] == ['k_gru_h16 + k_h1_frag']


@pytest.mark.parametrize('slot_base', [0, 5])
def test_row_counts(hs, slot_base):
    """cnt 1, 31, 32, 33, 70: one row, a ragged single tile, a full one, one row in a second tile, a ragged third"""
    rs = np.random.RandomState(100 + hs.L + slot_base)
    for cnt in (70, 1, 31, 32, 33):
        hs.encode(ids_of('mixed', cnt, hs.L, rs), slot_base)


@pytest.mark.parametrize('pattern', ['none', 'allzero', 'common', 'mixed', 'middle', 'last'])
def test_prefix_patterns(hs, pattern):
    rs = np.random.RandomState(200 + hs.L)
    hs.encode(ids_of(pattern, 70, hs.L, rs), 5)
    hs.encode(ids_of(pattern, 33, hs.L, rs), 0)


def test_second_encode_into_overlapping_slots(hs):
    """long histories first, then shorter ones (longer zero prefix) over part of the same slots: no stale fragment rows"""
    rs = np.random.RandomState(300 + hs.L)
    hs.encode(ids_of('none', 70, hs.L, rs), 0)
    hs.encode(ids_of('common', 40, hs.L, rs), 20)
    hs.encode(ids_of('allzero', 9, hs.L, rs), 30)


def test_whole_forward_on_top_of_the_fused_fragment_copy():
    """group 1 and group 9 forwards (k_din_x reads the fragment copy, k_augru_x<.., PAD> reads lead[]): default against gru_h16_v1"""
    import torch
    from rl4rs_amd.nets.dien import init_dien_weights
    from rl4rs_amd.device import DeviceDien
    w = init_dien_weights(CFG, seed=8, emb_scale=0.5, bias_noise=0.2)
    rs = np.random.RandomState(7)
    n = 40
    seq0 = ids_of('mixed', n, 64, rs)
    seq1 = ids_of('common', n, 64, rs)
    seq1[n // 2:] = 0
    outs = []
    for kernels in ('', 'gru_h16_v1'):
        net = DeviceDien(dict(CFG, scorer_kernels=kernels), w, max_rows=9 * n, max_slots=n)
        net.encode(0, torch.from_numpy(seq0).cuda(), 0)
        net.encode(1, torch.from_numpy(seq1).cuda(), 0)
        sl = torch.arange(n, dtype=torch.int32).repeat(2, 1).contiguous().cuda()
        got = []
        for group in (1, 9):
            R = n * group
            r2 = np.random.RandomState(group)
            dense = torch.from_numpy(np.abs(r2.randn(R, 432) * 3).astype(np.float32)).cuda()
            cat = torch.from_numpy(r2.randint(0, 284, size=(R, 21)).astype(np.int32)).cuda()
            obs, p = net.forward(R, group, dense, cat, sl, True, True)
            got += [obs.clone(), p.clone()]
        net.check_status()
        net.close()
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
