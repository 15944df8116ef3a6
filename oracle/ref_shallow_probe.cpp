// oracle/ref_shallow_probe.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// One more extern "C" entry around the UNMODIFIED reference headers, in a library of its own (oracle/_ref/libt4refshallow.so): a
// checkout that finds an oracle/_ref/libt4ref.so built before this entry existed still gets it, because its target is new. The
// SeqSet it is handed was made by libt4ref.so (ref_seqset_new); both libraries are compiled from the same headers with the same
// flags, so the object's layout is the same. No reference source is copied.
#define private public
#include "SeqSet.hpp"
#undef private

// The two globals every reference TU must define (main.cpp:39-44).
int nucToNum[26] = {0, -1, 1, -1, -1, -1, 2, -1, -1, -1, -1, -1, -1,
                    0, -1, -1, -1, -1, -1, 3, -1, -1, -1, -1, -1, -1};
char numToNuc[26] = {'A', 'C', 'G', 'T'};

// SeqSet::ReleaseShallowContigs (SeqSet.hpp:10926-10936; main.cpp:1952-1955)
extern "C" void refx_release_shallow_contigs(void *h, int minCov) { ((SeqSet *)h)->ReleaseShallowContigs(minCov); }
