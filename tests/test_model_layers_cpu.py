"""The bookkeeping the model layers share (robustmvd_amd/blocks.py): the packed-weight cache and the max-|x| slot hand-out.  No device."""
import pytest
import torch
import torch.nn as nn

from robustmvd_amd.blocks import PackedWeights, Slots


class Owner(PackedWeights, nn.Module):
    """one conv and one BatchNorm; _pack counts its calls and returns a fresh object"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(2, 3, 3)
        self.bn = nn.BatchNorm2d(3)
        self.packs = 0

    def _pack(self):
        self.packs += 1
        return object()


class FoldingOwner(Owner):
    FOLDS_BN = "FoldingOwner"


@pytest.mark.parametrize("cls", [Owner, FoldingOwner])
def test_packed_weights_cache(cls):
    net = cls().eval()
    assert net._packed is None
    pk = net._prepare()
    assert net.packs == 1 and net._packed is pk
    assert net._prepare() is pk and net._prepare() is pk and net.packs == 1  # reused

    def repacks(change):
        before, n = net._prepare(), net.packs
        change()
        after = net._prepare()
        assert net._prepare() is after  # and cached again
        return after is not before and net.packs == n + 1

    with torch.no_grad():
        assert repacks(lambda: net.conv.weight.add_(1))        # a parameter written in place
        assert repacks(lambda: net.bn.bias.mul_(2))
        assert repacks(lambda: net.bn.running_var.add_(1))     # a BN buffer written in place
        assert repacks(lambda: net.bn.running_mean.fill_(3))
    assert repacks(lambda: net.load_state_dict(cls().state_dict()))
    assert repacks(lambda: net.to(torch.float64))              # every tensor on new storage
    assert not repacks(lambda: net.eval())                     # nothing changed
    assert not repacks(lambda: net.conv.weight.sum())


def test_bn_folding_owner_refuses_training_mode():
    net = FoldingOwner().eval()
    pk = net._prepare()
    net.train()
    assert net._prepare() is pk  # nothing to pack: the refusal belongs to the packing
    with torch.no_grad():
        net.bn.running_mean.add_(1)
    with pytest.raises(RuntimeError, match=r"^FoldingOwner HIP path folds BatchNorm running statistics: call \.eval\(\) first$"):
        net._prepare()
    with pytest.raises(RuntimeError, match="folds BatchNorm running statistics"):
        FoldingOwner().train()._prepare()
    assert net.eval()._prepare() is not pk


def test_other_owner_packs_in_training_mode():
    net = Owner().train()
    assert net._prepare() is net._prepare() and net.packs == 1


def test_the_models_owners_name_themselves_as_before():
    """the four BN-folding sites keep their messages; the other three have none"""
    import robustmvd_amd as R
    from robustmvd_amd import cvp_mvsnet as C, vis_mvsnet as V
    from robustmvd_amd.blocks import FeatureNet
    from robustmvd_amd.dispnet_engine import DispnetEngine
    for net, name in ((FeatureNet(), "FeatureNet"), (R.CostRegNet(), "CostRegNet"), (C.CVPCostRegNet(), "CVPCostRegNet"),
                      (V.Reg3d("reg1", final=False), "Vis-MVSNet's")):
        with pytest.raises(RuntimeError) as e:
            net.train()._prepare()
        assert str(e.value) == f"{name} HIP path folds BatchNorm running statistics: call .eval() first"
        assert net._packed is None
    assert C.FeaturePyramid.FOLDS_BN is None and V.SingleStage.FOLDS_BN is None and DispnetEngine.FOLDS_BN is None


def test_packed_from_other_modules():
    """an owner that is not the packed module (DispnetEngine over RobustMVD, SingleStage over its two final convolutions)"""
    class Outside(PackedWeights):
        def __init__(self, *modules):
            self.modules, self.packs = modules, 0

        def _packed_from(self):
            return self.modules

        def _pack(self):
            self.packs += 1
            return object()

    a, b, other = nn.Conv2d(1, 1, 1), nn.BatchNorm2d(1), nn.Conv2d(1, 1, 1)
    out = Outside(a, b)
    pk = out._prepare()
    with torch.no_grad():
        other.weight.add_(1)
    assert out._prepare() is pk and out.packs == 1
    with torch.no_grad():
        b.running_mean.add_(1)
    assert out._prepare() is not pk and out.packs == 2


def test_slots():
    slots = Slots(3, torch.device("cpu"))
    assert slots.buf.dtype == torch.float32 and slots.buf.tolist() == [0.0, 0.0, 0.0]
    taken = [slots.take() for _ in range(3)]
    assert all(t.shape == (1,) for t in taken)
    assert [t.data_ptr() for t in taken] == [slots.buf.data_ptr() + 4 * i for i in range(3)]  # consecutive views of the one buffer
    taken[1].fill_(5.0)
    assert slots.buf.tolist() == [0.0, 5.0, 0.0]
    with pytest.raises(RuntimeError, match="all 3 max-.x. slots"):
        slots.take()


def test_slots_adopt_and_zero_a_buffer():
    buf = torch.full((2,), 7.0)
    slots = Slots(buf=buf)
    assert slots.buf is buf and buf.tolist() == [0.0, 0.0]
    assert slots.take().data_ptr() == buf.data_ptr() and slots.take().data_ptr() == buf.data_ptr() + 4
    with pytest.raises(RuntimeError):
        slots.take()
