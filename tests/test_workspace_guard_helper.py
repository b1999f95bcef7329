"""CPU: tests/workspace_guard.py on CPU tensors -- placement, what check() reports and what it must not, and that torch.empty comes back."""
import pytest
import torch

import workspace_guard as wg

SMALL = 4096      # (a band of 4 KiB keeps these tests at microseconds; the GPU tests use the module's 4 MiB)


@pytest.mark.parametrize("nbytes", [1, 4, 255, 256, 257, 1000, 4099])
def test_banded_placement(nbytes):
    b = wg.banded(nbytes, "cpu", band=SMALL)
    assert b.interior.numel() == nbytes and b.head.numel() == SMALL and b.tail.numel() == SMALL
    assert b.interior.data_ptr() % 256 == 0
    assert b.head.data_ptr() + SMALL == b.interior.data_ptr()
    assert b.tail.data_ptr() == b.interior.data_ptr() + nbytes            # the very first byte behind the interior: no rounding
    assert bool((b.head == wg.BAND_BYTE).all()) and bool((b.tail == wg.BAND_BYTE).all())
    b.fill(0x7F)
    assert bool((b.interior == 0x7F).all())
    b.check()


def test_default_band_is_4_mib_on_each_side():
    b = wg.banded(12, "cpu")
    assert b.head.numel() == b.tail.numel() == 4 << 20 == wg.BAND
    b.check()


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (3, 5, 7)), (torch.bfloat16, (11,)), (torch.float16, (2, 3)), (torch.int32, (1,))])
def test_flush_puts_the_band_right_behind_the_last_element(dtype, shape):
    t = torch.arange(int(torch.tensor(shape).prod())).reshape(shape).to(dtype)
    c = wg.flush(t, 0xFF, band=SMALL)
    assert c.dtype == dtype and c.shape == t.shape and torch.equal(c, t) and c.is_contiguous()
    g = wg.guard_of(c)
    assert c.data_ptr() % 256 == 0 and g.tail.data_ptr() == c.data_ptr() + c.numel() * c.element_size()
    assert g.band_byte == 0xFF and bool((g.tail == 0xFF).all())
    g.check()


@pytest.mark.parametrize("where,offset", [("tail", 0), ("tail", 1), ("tail", 255), ("tail", SMALL - 1), ("head", -1), ("head", -256), ("head", -SMALL)])
def test_a_planted_band_write_is_reported_with_its_offset(where, offset):
    b = wg.banded(1000, "cpu", band=SMALL).fill(0xFF)
    (b.tail if where == "tail" else b.head)[offset] = 0x00
    with pytest.raises(wg.BandError) as e:
        b.check("planted")
    msg = str(e.value)
    assert f"offset {offset} from the interior's {'end' if where == 'tail' else 'start'}" in msg, msg
    assert ("trailing" if where == "tail" else "leading") in msg and "planted" in msg


def test_the_first_changed_byte_is_the_one_named():
    b = wg.banded(64, "cpu", band=SMALL)
    b.tail[40] = 1
    b.tail[7] = 2
    with pytest.raises(wg.BandError, match=r"offset 7 from the interior's end .*2 band bytes changed"):
        b.check()


def test_writes_into_the_interior_are_not_reported():
    b = wg.banded(1000, "cpu", band=SMALL).fill(0x00)
    b.interior[0] = 0xA5
    b.interior[999] = 0x5A
    b.interior.view(torch.float32)[:250] = float("nan")
    b.check()
    t = wg.filled((5, 3), torch.float32, "cpu", 0xFF, band=SMALL)
    assert bool(torch.isnan(t).all())
    t.zero_()
    wg.guard_of(t).check()


def test_fill_bytes_mean_what_the_table_says():
    for dtype, ff, sf in ((torch.float32, "nan", 3.39e38), (torch.bfloat16, "nan", 3.39e38), (torch.float16, "nan", "nan")):
        a, b, z = (wg.filled((4,), dtype, "cpu", f, band=SMALL) for f in (0xFF, 0x7F, 0x00))
        assert bool(torch.isnan(a).all()) and bool((z == 0).all())
        if sf == "nan":
            assert bool(torch.isnan(b).all())
        else:
            assert bool(torch.isfinite(b).all()) and abs(float(b[0]) / sf - 1) < 0.01
    assert int(wg.filled((1,), torch.int32, "cpu", 0xFF, band=SMALL)[0]) == -1
    assert int(wg.filled((1,), torch.int32, "cpu", 0x7F, band=SMALL)[0]) == 2139062143


def test_guarded_allocations_hands_out_poisoned_flush_tensors_and_checks_them():
    real = torch.empty
    with wg.guarded_allocations(band=SMALL) as made:
        assert torch.empty is not real
        a = torch.empty(3, 5)
        b = torch.empty((2, 7), dtype=torch.bfloat16, device="cpu")
        c = torch.empty(torch.Size([4]), dtype=torch.int32)
        d = torch.empty(0)
        assert a.shape == (3, 5) and a.dtype == torch.float32 and bool(torch.isnan(a).all())
        assert b.shape == (2, 7) and b.dtype == torch.bfloat16 and bool(torch.isnan(b).all())
        assert c.dtype == torch.int32 and bool((c == -1).all()) and d.numel() == 0
        assert len(made) == 4
        assert wg.guard_of(a).tail.data_ptr() == a.data_ptr() + 60
        a.zero_()
    assert torch.empty is real


def test_guarded_allocations_reports_a_store_past_an_output():
    real = torch.empty
    with pytest.raises(wg.BandError, match="offset 2 from the interior's end"):
        with wg.guarded_allocations(band=SMALL):
            y = torch.empty(10, dtype=torch.uint8)
            wg.guard_of(y).tail[2] = 0
    assert torch.empty is real


def test_guarded_allocations_restores_torch_empty_when_the_body_raises():
    real = torch.empty
    with pytest.raises(KeyError):
        with wg.guarded_allocations(band=SMALL):
            y = torch.empty(10, dtype=torch.uint8)
            wg.guard_of(y).tail[0] = 0          # (a tripped band does not mask the body's own exception)
            raise KeyError("body")
    assert torch.empty is real
