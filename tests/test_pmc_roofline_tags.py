"""tools/pmc_roofline.py sorts kernel families under bench.py's roofline tags by substrings of their names.  The two backbone instances of
K3's linear_kernel are told apart by the tail of their template list, so a new template argument on linear_kernel moves them silently
under `k3_linear` unless the patterns follow: the patterns are checked here against the template list in the source."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _tags(family):
    import pmc_roofline as P
    return [t for t, pats in P.TAG_FAMILIES.items()
            if any(p in family for p in pats) and not any(x in family for x in P.TAG_EXCLUDE.get(t, []))]


def test_backbone_patterns_follow_linear_kernels_template_list():
    import pmc_roofline as P
    src = open(os.path.join(ROOT, 'geoformer_amd', 'csrc', 'k3_linear.hip')).read()
    m = re.search(r'template <([^>]*)>\s*__global__[^\n]*void linear_kernel\(', src)
    params = [p.strip() for p in m.group(1).split(',')]
    assert [p.split()[1] for p in params[:4]] == ['T', 'NB', 'EPI', 'CONVX'] and all(p.endswith('= false') for p in params[3:])
    tail = ', false' * (len(params) - 4) + '>'                       # every flag behind CONVX is off in the backbone's instances
    assert P.K3_UPADD == ', 4, 5, true' + tail and P.K3_CONV1X1 == ', 4, 0, true' + tail


def test_k3_kernel_names_land_under_their_tags():
    import pmc_roofline as P
    # as rocprofv3 reports them: _Float16 instances stay mangled, the others come demangled
    assert _tags(P.family('_ZN12_GLOBAL__N_113linear_kernelIDF16_Li4ELi5ELb1ELb0EEEvNS_7LinArgsE')) == ['k3_upadd']
    assert _tags(P.family('_ZN12_GLOBAL__N_113linear_kernelIDF16_Li4ELi0ELb1ELb0EEEvNS_7LinArgsE')) == ['conv1x1']
    assert _tags(P.family('void (anonymous namespace)::linear_kernel<__bf16, 4, 5, true, false>((anonymous namespace)::LinArgs)')) == ['k3_upadd']
    for name in ('_ZN12_GLOBAL__N_113linear_kernelIDF16_Li4ELi0ELb0ELb0EEEvNS_7LinArgsE',          # gf_linear
                 '_ZN12_GLOBAL__N_113linear_kernelIDF16_Li4ELi0ELb0ELb1EEEvNS_7LinArgsE',          # gf_linear_rows: window and coarse rows
                 '_ZN12_GLOBAL__N_113linear_kernelIDF16_Li8ELi0ELb0ELb1EEEvNS_7LinArgsE',          # gf_linear_rows: k | v at the inlier tokens
                 '_ZN12_GLOBAL__N_116linear_kernel_w2IDF16_Li0EEEvNS_7LinArgsE'):
        assert _tags(P.family(name)) == ['k3_linear'], name
