"""Every leading dimension and stride of include/spt_hip.h's prototypes (a parameter named `ld*`,
`*stride*` or `*pitch*`), and every such field of a descriptor a launching entry takes, has a padded case in test_gpu_placement.PADDED, or a reason in its TIGHT_ONLY
why no caller of naive_gpt.ext can pass another value than the tight one."""
import os
import re

import test_gpu_placement as placement
from test_contract_refusals import HEADER, prototypes

EXT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'spt-proto_amd', 'naive_gpt',
                   'ext.py')
NAMED = re.compile(r'ld\w*|\w*stride\w*|\w*pitch\w*')


def strided_parameters():
    found = {(entry, p) for entry, params in prototypes().items() for p in params if NAMED.fullmatch(p)}
    # the descriptors: fields of `typedef struct Name { ... } Name;`, under every entry that takes a
    # `const Name *` and a stream (the host-only spt_grouped_gemm_image_path* launch nothing)
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for m in re.finditer(r'typedef struct (\w+) \{(.*?)\} \1;', text, flags=re.S):
        fields = [f for decl in m.group(2).split(';') for f in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
        takers = [e.group(1) for e in re.finditer(r'\b(spt_\w+)\s*\(([^)]*)\)', text)
                  if re.search(r'\b' + m.group(1) + r' \*', e.group(2)) and 'stream' in e.group(2)]
        assert takers and fields, m.group(1)
        found |= {(e, f) for e in takers for f in fields if NAMED.fullmatch(f)}
    return sorted(found)


def test_every_leading_dimension_is_padded_or_tight_for_a_reason():
    params = strided_parameters()
    assert len(params) > 60 and ('spt_tall_tn', 'ldw') in params and ('spt_rotary', 'out_stride') in params
    assert ('spt_grouped_gemm_fused_w16', 'ldo') in params and ('spt_grouped_gemm_bf16_ext', 'lda2') in params
    tables = set(placement.PADDED) | set(placement.TIGHT_ONLY)
    missing = [p for p in params if p not in tables]
    assert not missing, 'leading dimensions without a PADDED case or a TIGHT_ONLY reason: {}'.format(missing)
    stale = sorted(tables - set(params))
    assert not stale, 'PADDED / TIGHT_ONLY name parameters the header no longer has: {}'.format(stale)
    both = sorted(set(placement.PADDED) & set(placement.TIGHT_ONLY))
    assert not both, both
    assert all(isinstance(r, str) and len(r.strip()) > 20 for r in placement.TIGHT_ONLY.values()), 'an empty reason'
    assert all(callable(c) and c.__name__.startswith('_pad_') for c in placement.PADDED.values())


def test_tight_only_values_are_not_read_from_a_tensor():
    """Keeps TIGHT_ONLY honest: in the binding's call of such an entry the argument is no `.stride(...)`
    of a tensor and no name a caller passes."""
    source = open(EXT).read()
    for (entry, param), _ in placement.TIGHT_ONLY.items():
        at = prototypes()[entry].index(param)
        calls = [m.end() for m in re.finditer(r'lib\.' + entry + r'\(', source)]
        assert calls, entry
        for start in calls:
            depth, i, args, cur = 1, start, [], ''
            while depth:
                c = source[i]
                depth += c in '([' 
                depth -= c in ')]'
                if c == ',' and depth == 1:
                    args.append(cur)
                    cur = ''
                elif depth:
                    cur += c
                i += 1
            args.append(cur)
            arg = ' '.join(args[at].split())
            assert 'stride' not in arg, '{} {}: the binding passes {!r}'.format(entry, param, arg)
            assert re.fullmatch(r'0|width|k \* n|x0\.numel\(\)', arg), \
                '{} {}: the binding passes {!r}, which a caller may choose'.format(entry, param, arg)
