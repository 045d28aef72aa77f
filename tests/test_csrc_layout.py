"""Layout of the host code under csrc/ (a text scan: no library, no GPU). What one .hip file calls in another is declared once, in
lvae_host.h, which both sides include: a local re-declaration or a second copy of a struct can drift from the original without a
compiler or linker error."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ladder-vae-pytorch_amd', 'csrc')


def sources(*suffixes):
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(suffixes)}


def strip(text):
    """comments, preprocessor lines and the contents of literals removed; line breaks kept"""
    text = re.sub(r'//[^\n]*|/\*.*?\*/', lambda m: '\n' * m.group(0).count('\n'), text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', '""', text)
    return re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', lambda m: '\n' * m.group(0).count('\n'), text, flags=re.M)


def statements(text):
    """(kind, head, line) of every statement at namespace scope: kind 'decl' ends in ';', kind 'def' opens a body (which is skipped).
    `namespace ... {` and `extern "C" {` are looked through."""
    out, head, start, line, parens = [], [], 1, 1, 0
    stack = []  # one entry per open brace: True = a namespace / linkage block, False = a body
    for c in strip(text):
        line += c == '\n'
        if False in stack:  # inside a body
            if c in '{}':
                stack.append(False) if c == '{' else stack.pop()
            continue
        if not head:
            if c.isspace():
                continue
            start = line
        parens += (c == '(') - (c == ')')
        if parens == 0 and c in '{};':
            text_ = ' '.join(''.join(head).split())
            head = []
            if c == '{':
                stack.append(re.match(r'(namespace\b[^=]*|extern "")$', text_) is not None)
                if not stack[-1]:
                    out.append(('def', text_, start))
            elif c == '}':
                stack.pop()
            elif text_:
                out.append(('decl', text_, start))
            continue
        head.append(c)
    return out


# `... name(parameters)`, also `name<4>(parameters)` of a specialisation; no initialiser, no typedef / using / static_assert / explicit instantiation
FUNCTION = re.compile(r'(?:template\s*<[^<>]*>\s*)?(?!typedef\b|using\b|static_assert\b|template\b)[^=()]*?\b([A-Za-z_]\w*)\s*(?:<[^<>()]*>)?\s*\(.*\)(?:\s*const)?$')
STRUCT = re.compile(r'(?:template\s*<.*>\s*)?(?:struct|class|union)\s+(?:alignas\s*\(\w+\)\s*|__attribute__\s*\(\(.*?\)\)\s*)*([A-Za-z_]\w*)(?:\s*:[^;(]*)?$')


def test_scanner_tells_declarations_from_definitions():
    sample = '''
    #define M(x) \\
      void hidden(int);
    namespace lvae {
    int declared_only(const char* s,
                      int n);   // void in_comment(int);
    static int forward(int);
    static int forward(int a) { return a; }
    template <int V> __device__ float& at(float& v, int j);
    template <> __device__ float& at<4>(float& v, int) { return v; }
    constexpr int kValue = f(3);
    struct Args { int a; void member(int); };
    template <int N> struct alignas(16) Wide { float v[N]; };
    template __global__ void kern<4>(Args);
    }  // namespace lvae
    extern "C" int lvae_entry(void* p) { struct Local { int q; }; return 0; }
    '''
    st = statements(sample)
    decls = [FUNCTION.match(h).group(1) for k, h, _ in st if k == 'decl' and FUNCTION.match(h)]
    defs = [FUNCTION.match(h).group(1) for k, h, _ in st if k == 'def' and FUNCTION.match(h)]
    structs = [STRUCT.match(h).group(1) for k, h, _ in st if k == 'def' and STRUCT.match(h)]
    assert decls == ['declared_only', 'forward', 'at']
    assert defs == ['forward', 'at', 'lvae_entry']
    assert structs == ['Args', 'Wide']


def test_no_hip_file_declares_a_function_it_does_not_define():
    bad = []
    for f, text in sources('.hip').items():
        st = statements(text)
        defined = {FUNCTION.match(h).group(1) for k, h, _ in st if k == 'def' and FUNCTION.match(h)}
        assert defined, f  # the scanner found this file's functions at all
        for k, h, line in st:
            m = FUNCTION.match(h) if k == 'decl' else None
            if m and m.group(1) not in defined:
                bad.append('%s:%d: %s;' % (f, line, h))
    assert not bad, 'declare what another file defines in lvae_host.h, once:\n' + '\n'.join(bad)


def test_every_struct_is_defined_in_one_file():
    where = {}
    for f, text in sources('.hip', '.h', '.inc').items():
        for k, h, _ in statements(text):
            m = STRUCT.match(h) if k == 'def' else None
            if m and 'template <>' not in h and 'template<>' not in h:  # (a specialisation repeats its template's name)
                where.setdefault(m.group(1), set()).add(f)
    assert len(where) > 30 and 'ReduceArgs' in where and 'ConvPlan' in where  # the scanner sees the structs at all
    twice = {name: sorted(files) for name, files in where.items() if len(files) > 1}
    assert not twice, 'a struct that crosses files is defined in lvae_host.h, once: %r' % twice


def test_cross_file_interface_is_in_lvae_host_h():
    host = statements(sources('.h')['lvae_host.h'])
    declared = [FUNCTION.match(h).group(1) for k, h, _ in host if k == 'decl' and FUNCTION.match(h)]
    assert len(declared) == len(set(declared)) and len(declared) >= 38, 'each function once'
    hips = sources('.hip')
    defined = {f: {FUNCTION.match(h).group(1) for k, h, _ in statements(text) if k == 'def' and FUNCTION.match(h)} for f, text in hips.items()}
    code = {f: strip(text) for f, text in hips.items()}
    for name in declared:  # defined by one .hip (which includes the header, so that a changed signature cannot compile) and called from another
        definers = [f for f in hips if name in defined[f]]
        assert len(definers) == 1, (name, definers)
        users = [f for f in hips if re.search(r'\b%s\s*\(' % name, code[f])]
        assert len(users) >= 2, '%s is used by %s only: keep it static there' % (name, definers[0])
        for f in users:
            assert '#include "lvae_host.h"' in hips[f], (name, f)


def test_only_the_launcher_raises_a_kernels_lds_limit():
    for f, text in sources('.hip', '.h', '.inc').items():
        for word in ('hipFuncSetAttribute', 'attr_set'):
            assert (word in strip(text)) == (f == 'lvae_host.h'), (f, word)
    assert re.search(r'-Wl,--no-undefined', open(os.path.join(CSRC, 'Makefile')).read()), 'a missing definition has to fail the link'
