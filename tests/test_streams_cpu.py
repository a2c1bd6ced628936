"""Completeness of the table of stream cases (tests/stream_cases.py, run by tests/test_gpu_streams.py) against the header: every prototype of
include/stratego_mi355x.h that takes a `void *stream` is a row of the table or stands in the exclusion list below with its reason, and the header's list of entry points that wait for
the device is what the table marks may_wait.  A new entry point cannot ship without a stream case."""
import os
import re

from tests.stream_cases import CASES

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'stratego_mi355x.h')

# stream-taking entry points without a case, each with its reason
EXCLUDED = {
    'sgx_time_observe': 'a measurement: times its launches with events and synchronises the stream by design (the header lists it as waiting)',
    'sgx_mem_probe': 'a measurement of a memory range, no handle: synchronises the stream by design (listed as waiting)',
    'sgx_store_probe': 'a measurement of a memory range, no handle: synchronises the stream by design (listed as waiting)',
    'sgx_alloc_outputs': 'a measurement and placement tool: allocates, times candidates and waits for the device by design (listed as waiting)',
}


def _header():
    with open(HEADER) as f:
        return f.read()


def prototypes(text):
    """name -> parameter list of every function the header declares (comments removed first)."""
    code = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'\b(sgx_\w+)\s*\(([^;{}]*)\)\s*;', code)}


def stream_takers(text):
    return {name for name, params in prototypes(text).items() if re.search(r'\bvoid\s*\*\s*stream\b', params)}


def waiting_list(text):
    """The names of the header's sentence 'the entry points that wait for the device are ... ;'."""
    m = re.search(r'the entry points that wait for the device are(.*?);', text, flags=re.S)
    assert m, "the header no longer has its list of waiting entry points"
    return set(re.findall(r'sgx_\w+', m.group(1)))


def test_the_parser_reads_the_header():
    text = _header()
    protos = prototypes(text)
    assert 'sgx_step' in protos and 'sgx_create' in protos and 'sgx_state_keys' in protos
    takers = stream_takers(text)
    assert {'sgx_step', 'sgx_count_moves', 'sgx_store_probe', 'sgx_playout_weighted', 'sgx_get_env_info'} <= takers
    assert not takers & {'sgx_create', 'sgx_destroy', 'sgx_set_start_pool', 'sgx_num_envs'}
    assert len(takers) >= 31
    # a prototype that is added is found: the parser is not a list of names
    grown = text.replace('#ifdef __cplusplus\n}', 'int sgx_new_call(sgx_env *h, const int32_t *x_dev,\n    void *stream);\n#ifdef __cplusplus\n}', 1)
    assert stream_takers(grown) - takers == {'sgx_new_call'}


def test_every_stream_taking_entry_point_has_a_case_or_an_exclusion():
    takers = stream_takers(_header())
    covered = {e for c in CASES for e in c.entries}
    assert not covered - takers, "cases name entry points that take no stream: %s" % sorted(covered - takers)
    assert not set(EXCLUDED) - takers, "exclusions that are no stream-taking prototypes: %s" % sorted(set(EXCLUDED) - takers)
    assert not covered & set(EXCLUDED), "excluded AND covered: %s" % sorted(covered & set(EXCLUDED))
    missing = takers - covered - set(EXCLUDED)
    assert not missing, ("entry points that take a stream but have neither a case in tests/stream_cases.py nor an exclusion with a reason "
                         "here: %s" % sorted(missing))
    assert all(len(reason) > 20 for reason in EXCLUDED.values())


def test_the_headers_waiting_list_is_what_the_table_marks():
    text = _header()
    waits, takers, protos = waiting_list(text), stream_takers(text), prototypes(text)
    assert waits <= set(protos), "the waiting list names what the header does not declare: %s" % sorted(waits - set(protos))
    may_wait = {e for c in CASES if c.may_wait for e in c.entries}
    always_async = {e for c in CASES if not c.may_wait for e in c.entries}
    assert not may_wait & always_async, "marked may_wait in one row and asynchronous in another: %s" % sorted(may_wait & always_async)
    # of the stream-taking entry points, the header's list is the excluded measurement tools plus the rows marked may_wait -- both ways
    assert waits & takers == may_wait | set(EXCLUDED), (sorted(waits & takers), sorted(may_wait | set(EXCLUDED)))
