"""The 'bf16_fp16' precision mode (bf16 backbone, fp16 matching path) where no GPU is needed: the mode table of
GeoFormer.set_precision and the command line's parser."""
import pytest
import torch


def _model(precision):
    from geoformer_amd.model.cvpr_ds_config import get_default_cfg
    from geoformer_amd.model.full_model import GeoFormer
    from geoformer_amd.model.geo_config import get_cfg_model
    gc = get_cfg_model()
    gc['precision'] = precision
    return GeoFormer(get_default_cfg(), gc)


def _backbone_dtypes(m):
    return {p.dtype for p in m.backbone.parameters()}


def test_mode_from_config_and_back():
    m = _model('bf16_fp16')
    assert m.precision == 'bf16_fp16'
    assert m.compute_dtype == torch.float16 and m.backbone_dtype == torch.bfloat16
    assert _backbone_dtypes(m) == {torch.bfloat16}
    # the matching path's own parameters stay fp32 masters (their 16-bit copies are made per compute dtype on first use)
    assert {p.dtype for p in m.loftr_coarse.parameters()} == {torch.float32}
    assert m.set_precision('fp16') is m
    assert m.precision == 'fp16' and m.compute_dtype == m.backbone_dtype == torch.float16
    assert _backbone_dtypes(m) == {torch.float16}
    m.set_precision('bf16_fp16')
    assert (m.precision, m.compute_dtype, m.backbone_dtype) == ('bf16_fp16', torch.float16, torch.bfloat16)
    assert _backbone_dtypes(m) == {torch.bfloat16}


def test_explicit_backbone_dtype_still_overrides():
    m = _model('fp32')
    m.set_precision('bf16_fp16', backbone_dtype=torch.float32)
    assert m.precision == 'bf16_fp16' and m.compute_dtype == torch.float16 and m.backbone_dtype == torch.float32
    assert _backbone_dtypes(m) == {torch.float32}
    m.set_precision('bf16')                       # the single-dtype modes are what they were
    assert m.compute_dtype == m.backbone_dtype == torch.bfloat16 and _backbone_dtypes(m) == {torch.bfloat16}


def test_unknown_mode_names_the_valid_ones():
    m = _model('fp32')
    with pytest.raises(ValueError) as e:
        m.set_precision('nope')
    for name in ('fp32', 'fp16', 'bf16', 'bf16_fp16'):
        assert repr(name) in str(e.value), str(e.value)
    assert m.precision == 'fp32' and m.compute_dtype == torch.float32      # a refused name changes nothing


def test_state_dict_reload_keeps_the_backbone_dtype():
    m = _model('bf16_fp16')
    m.load_state_dict(_model('fp32').state_dict())
    assert _backbone_dtypes(m) == {torch.bfloat16} and m.compute_dtype == torch.float16


@pytest.mark.parametrize('cmd', [['match', 'a.ppm', 'b.ppm'], ['hpatches', '/data/hpatches']])
def test_command_line_parser_accepts_the_mode(cmd):
    from geoformer_amd import matcher as MT
    ap = MT.build_parser()
    assert ap.parse_args(cmd + ['--precision', 'bf16_fp16']).precision == 'bf16_fp16'
    assert ap.parse_args(cmd).precision == 'fp16'                          # the default is unchanged
    with pytest.raises(SystemExit):
        ap.parse_args(cmd + ['--precision', 'fp16_bf16'])
