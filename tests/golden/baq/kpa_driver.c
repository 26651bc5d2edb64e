/* kpa_driver.c -- the driver tests/golden/make_baq_fixtures.py links with the reference's own samtools/kprobaln.c (which
 * is compiled from the reference tree into a temporary directory and never copied here).  stdin: per case one line
 * "l_ref l_query bw ref query qual", the three arrays as hex strings ("-" for an empty one); stdout: per case one line
 * "state... | q-as-hex", what kpa_glocal filled. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kprobaln.h"

static void unhex(const char *s, uint8_t *out, int n)
{
    int i;
    for (i = 0; i < n; ++i) {
        unsigned v = 0;
        sscanf(s + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

int main(void)
{
    static char a[1 << 16], b[1 << 16], c[1 << 16];
    int l_ref, l_query, bw, i;
    while (scanf("%d %d %d %65535s %65535s %65535s", &l_ref, &l_query, &bw, a, b, c) == 6) {
        uint8_t *ref = calloc(l_ref + 1, 1), *query = calloc(l_query + 1, 1), *qual = calloc(l_query + 1, 1);
        int *state = calloc(l_query + 1, sizeof(int));
        uint8_t *q = calloc(l_query + 1, 1);
        kpa_par_t conf = kpa_par_def;
        conf.bw = bw;
        unhex(a, ref, l_ref);
        unhex(b, query, l_query);
        unhex(c, qual, l_query);
        kpa_glocal(ref, l_ref, query, l_query, qual, &conf, state, q);
        for (i = 0; i < l_query; ++i) printf("%d ", state[i]);
        printf("| ");
        for (i = 0; i < l_query; ++i) printf("%02x", q[i]);
        printf("\n");
        free(ref); free(query); free(qual); free(state); free(q);
    }
    return 0;
}
