"""The environment knobs of the engine: libhscmp reads the environment in one function,
read_knobs, and the section's table names exactly the knobs the package reads."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'hierarchical-sparse-coding_amd')


def _strip_comments(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _native_sources():
    for dirpath, _, files in os.walk(os.path.join(PKG, 'csrc')):
        for f in sorted(files):
            if f.endswith(('.h', '.hip')):
                yield f, _strip_comments(open(os.path.join(dirpath, f)).read())


def _split_read_knobs():
    """(body of read_knobs, every native source with that body cut out)"""
    body, rest = None, []
    for name, text in _native_sources():
        m = re.search(r'\bKnobs\s+read_knobs\s*\(\s*\)\s*\{', text)
        if m:
            assert body is None, 'read_knobs is defined twice'
            depth, i = 1, m.end()
            while depth:
                depth += {'{': 1, '}': -1}.get(text[i], 0)
                i += 1
            body = text[m.end():i]
            text = text[:m.start()] + text[i:]
        rest.append((name, text))
    assert body is not None, 'read_knobs not found'
    return body, rest


def _table_knobs():
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = text[text.index('### 3.4 '):]
    section = section[:section.index('\n#', 1)]
    names = set()
    for line in section.splitlines():
        if line.startswith('| `'):
            names.update(re.findall(r'`(HSCMP_[A-Z0-9_]+)', line.split('|')[1]))
    return names


def test_read_knobs_is_the_only_reader_of_the_environment():
    body, rest = _split_read_knobs()
    assert 'getenv(' in body
    for name, text in rest:
        assert 'getenv(' not in text, '%s reads the environment outside read_knobs' % name


def test_design_table_lists_every_knob():
    body, _ = _split_read_knobs()
    native = set(re.findall(r'getenv\(\s*"(HSCMP_[A-Z0-9_]+)"\s*\)', body))
    python = set()
    for f in sorted(os.listdir(PKG)):
        if f.endswith('.py'):
            text = open(os.path.join(PKG, f)).read()
            python.update(re.findall(r'os\.environ(?:\.get\(|\[)\s*[\'"](HSCMP_[A-Z0-9_]+)[\'"]', text))
    assert native and python
    assert native | python == _table_knobs()
