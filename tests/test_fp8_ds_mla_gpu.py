"""serialize="fp8_ds_mla" through the HIP kernels on MI355X.

kvc_gather_fp8_mla / kvc_scatter_fp8_mla (one wave per token row, four rows
per workgroup) must write and read exactly the reference bytes of
test_fp8_ds_mla.py, the bytes host mode writes. Shapes are the smallest at
which the kernels can go wrong:

  rows  layers x blocks
  1     2 x 4      one live wave in a workgroup, three waves with no row
  5     2 x 4      a second workgroup per tile that is three-quarters empty
  16    4 x 16     the DeepSeek preset's tile (18 KiB), several slices
  64    2 x 4      16 workgroups per tile
  1     2 x 160    ids through the device id buffer instead of the kernarg
  16    16 x 128   2048 tiles: one slice per tile, four trips of the row loop
"""
import pytest
import torch

from test_fp8_ds_mla import (
    assert_loaded,
    copier_roundtrip,
    mla_case,
    mla_engine,
    roundtrip,
    wait_finished,
)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 4), (5, 2, 4), (16, 4, 16), (64, 2, 4), (1, 2, 160),
          (16, 16, 128)]


def _dev(case):
    return [p.cuda() for p in case[0]]


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d-l%d-n%d" % s)
def test_gpu_roundtrip_matches_reference(tmp_path, shape, copy_path):
    case = mla_case(*shape)
    roundtrip(_dev(case), tmp_path, case, copy_path)


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("kw", [dict(dtype=torch.float16),
                                dict(checksum=True)], ids=["fp16", "checksum"])
def test_gpu_fp16_and_checksum(tmp_path, kw, copy_path):
    case = mla_case(5, 2, 4, kw.get("dtype", torch.bfloat16))
    roundtrip(_dev(case), tmp_path, case, copy_path,
              checksum=kw.get("checksum", False))


def test_gpu_loads_file_written_in_host_mode(tmp_path):
    case = mla_case(5, 2, 4)
    _, ids, _, loaded = case
    roundtrip([p.clone() for p in case[0]], tmp_path, case, "host")
    pages = [torch.zeros_like(p, device="cuda") for p in case[0]]
    _, _, _, load = mla_engine(pages, tmp_path, len(ids), "staged")
    load.transfer_async([0xD5], {0: ids})
    assert wait_finished(load)[0].success
    assert_loaded(pages, ids, loaded)


def test_gpu_block_copier_matches_reference():
    case = mla_case(5, 2, 4)
    copier_roundtrip(_dev(case), case)
