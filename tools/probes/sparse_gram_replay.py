"""Replay of ttr_sparse_gram's index logic on the CPU (no device): the tiling of csrc/ttr_sparse.hip (mode index, j range,
(a, b) tile, part), the forward scan of a block's column for its partners, the per-part partial matrices and the mirroring
finish, written as plain loops and compared with D D^T on the block tables of tests/test_sparse_gpu.py.

    python tools/probes/sparse_gram_replay.py

Prints, per table, the largest difference from D D^T and whether an element was left unwritten."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
kCh,kJt,kRt,kAcc,kT=32,64,32,8,256
def geom(r,I,nb):
    TA=min(r,kRt); jt=kAcc*kT//(TA*TA); jt=min(jt,kJt,I); jt=max(jt,1)
    nTA=-(-r//TA); nJ=-(-I//jt); p=min(16,-(-max(nb,1)//(I*2048)))
    return TA,jt,nTA,nJ,p
def gram(r,I,colptr,blk_i,blkcol,ilist,iptr,V):
    nb=len(blk_i); C=len(colptr)-1; TA,Jt,nTA,nJ,parts=geom(r,I,nb); TB=TA; nTB=nTA; n=r*I
    Gp=np.full((parts,n,n),np.nan)
    for part in range(parts):
      for i in range(I):
        for bx in range(nJ*nTA*nTB):
            t=bx; tb=t%nTB; t//=nTB; ta=t%nTA; tj=t//nTA
            j0,a0,b0=tj*Jt,ta*TA,tb*TB
            jn,an,bn=min(Jt,I-j0),min(TA,r-a0),min(TB,r-b0)
            if j0+jn-1<i: continue
            E=Jt*TA*TB; acc=np.zeros(E)
            qlo,qhi=iptr[i],iptr[i+1]; ln=max(qhi-qlo,0); per=(ln+parts-1)//parts
            qs=qlo+part*per; qe=min(qs+per,qhi)
            q0=qs
            while q0<qe:
                nch=min(kCh,qe-q0)
                partner=-np.ones((kCh,kJt),int); vi=np.zeros((kCh,kRt))
                for ch in range(nch):
                    B=ilist[q0+ch]
                    for aa in range(an): vi[ch,aa]=V[B,a0+aa]
                    c=blkcol[B]; end=min(colptr[c+1],nb)
                    for Bp in range(B,end):
                        j=blk_i[Bp]
                        if j>=j0+jn: break
                        if j>=j0 and j>=i: partner[ch,j-j0]=Bp
                for e in range(E):
                    bb=e%TB; aa=(e//TB)%TA; jj=e//(TB*TA)
                    if jj<jn and aa<an and bb<bn:
                        for ch in range(nch):
                            p=partner[ch,jj]
                            if p>=0: acc[e]+=vi[ch,aa]*V[p,b0+bb]
                q0+=kCh
            for e in range(E):
                bb=e%TB; aa=(e//TB)%TA; jj=e//(TB*TA)
                if jj<jn and aa<an and bb<bn:
                    Gp[part,(a0+aa)*I+i,(b0+bb)*I+j0+jj]=acc[e]
    G=np.zeros((n,n))
    for R in range(n):
        for Cc in range(n):
            src=(R,Cc) if (Cc%I)>=(R%I) else (Cc,R)
            G[R,Cc]=sum(Gp[p][src] for p in range(parts))
    return G
from test_sparse_gpu import table
for r,I,f in [(1,5,"one_block"),(3,5,"one_full_column"),(3,16,"absent_index"),(17,1,"one_column"),(33,3,"one_full_column"),(2,67,"one_full_column")]:
    colptr,blk_i,blkcol,V,D,mm=table(r,I,f,torch.float64,1)
    order=torch.sort(blk_i,stable=True).indices
    iptr=torch.cat([torch.zeros(1,dtype=torch.int64),torch.cumsum(torch.bincount(blk_i,minlength=I),0)])
    G=gram(r,I,colptr.numpy(),blk_i.numpy(),blkcol.numpy(),order.numpy(),iptr.numpy(),V.numpy())
    ref=(D@D.t()).numpy()
    print(r,I,f,np.abs(G-ref).max(), np.isnan(G).any())
